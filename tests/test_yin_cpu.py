"""YIN without a GPU: the float64 restatement (tests/yin_ref.py) against exact periodic structure and its own bounds, csrc/yin.hip
itself run on the host stand-in against the restatement (tests/yin_cases.py holds the cases the GPU file repeats), audio.f0_metrics,
the refusals, and the argument handling of the evaluate tool's wav mode."""
import contextlib
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import yin_cases as yc
import yin_ref as yr
from tacotron2_amd import audio, evaluate, native

CPU = torch.device("cpu")


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", yc.PERIODS)
def test_restatement_exact_period(P):
    geo = yc.DEFAULT
    L, hop = geo["frame_length"], geo["hop_length"]
    x = yr.periodic(P, 2560)
    ref = yr.analyse(x, **geo)
    assert ref["dprime"].shape == (11, 370) and (ref["tau_min"], ref["tau_max"]) == (27, 368)
    interior = [t for t in range(11) if t * hop - L // 2 >= 0 and t * hop + L // 2 <= len(x)]
    assert interior == list(range(2, 9))
    for t in interior:
        assert ref["voiced"][t] and ref["tau"][t] == P and ref["aperiodicity"][t] == 0.0
        assert abs(ref["tau"][t] + ref["shift"][t] - P) <= 0.5


def test_restatement_definitions():
    g = np.random.RandomState(1)
    x = g.randn(300).astype(np.float32)
    fr = yr.frames(x, 64, 16)
    assert fr.shape == (300 // 16 + 1, 64) and not fr[0, :32].any() and np.array_equal(fr[0, 32:], x[:32].astype(np.float64))
    assert np.array_equal(fr[5], x[48:112].astype(np.float64)) and not fr[-1, 32 + 300 - 288:].any()
    dp = yr.dprime(fr, 30)
    f = fr[5]
    d = [sum((f[j] - f[j + tau]) ** 2 for j in range(32)) for tau in range(1, 32)]
    for tau in (1, 2, 17, 31):
        assert abs(dp[5, tau] - d[tau - 1] * tau / sum(d[:tau])) <= 1e-12
    assert (dp[:, 0] == 1.0).all() and (dp[:, 1] == 1.0).all()
    # the rule: the first dip below the threshold, else the first argmin
    row = np.array([1.0, 1.0, 0.9, 0.5, 0.05, 0.3, 0.01, 0.2, 0.6])
    assert yr.choose(row, 2, 7, 0.1) == (4, True) and yr.choose(row, 5, 7, 0.1) == (6, True)
    assert yr.choose(row, 2, 7, 0.005) == (6, False) and yr.choose(np.ones(9), 2, 7, 0.1) == (2, False)
    assert yr.choose(np.array([1, 1, .05, .05, .05, 1.0]), 2, 4, 0.1) == (2, True)           # d'(tau) <= d'(tau + 1): a plateau's first
    # the refinement: the vertex of the parabola, 0 where the middle is no minimum or the three are equal
    assert yr.refine(0.4, 0.1, 0.4) == 0.0 and yr.refine(1.0, 1.0, 1.0) == 0.0 and yr.refine(0.1, 0.2, 0.3) == 0.0
    assert abs(yr.refine(0.3, 0.1, 0.5) - (-0.1 / 0.6)) <= 1e-15 and yr.refine(0.125, 0.125, 0.5) == -0.5
    assert yr.decided(row, 2, 7, 0.1, 1e-3) and not yr.decided(row, 2, 7, 0.05, 1e-3) and not yr.decided(np.ones(9), 2, 7, 0.1, 1e-3)
    assert abs(yr.bound(512, 368) - 1400 * 2.0 ** -24) < 1e-18


def test_restatement_leaves_out_at_most_a_tenth_of_the_glides():
    geo, voiced = yc.DEFAULT, 0
    for seed, x in enumerate(yc.glide_signals()):
        ref = yr.analyse(x, **geo)
        tol = yr.bound(ref["W"], ref["tau_max"])
        n = sum(yr.decided(row, ref["tau_min"], ref["tau_max"], geo["threshold"], tol) for row in ref["dprime"])
        assert ref["dprime"].shape[0] == 41 and 1 - n / 41 <= 0.10, (seed, n)
        voiced += int(ref["voiced"].sum())
    assert 60 <= voiced <= 6 * 41 - 60                                          # both kinds of frame are there


def test_metrics_restatement_by_hand():
    m = yr.metrics([100, 200, 300, 0], [1, 1, 1, 0], [100, 100, 600, 50], [1, 1, 0, 1])
    assert m["voiced_steps"] == 2 and m["vuv_error"] == 0.5 and m["gross_pitch_error"] == 0.5
    assert abs(m["f0_rmse_cents"] - np.sqrt(1200.0 ** 2 / 2)) <= 1e-9 and np.isnan(m["f0_corr"])      # fb constant
    m = yr.metrics([100, 200, 400], [1, 1, 1], [50, 100, 200], [1, 1, 1], path=[(0, 0), (1, 1), (2, 2)])
    assert abs(m["f0_rmse_cents"] - 1200.0) <= 1e-9 and abs(m["f0_corr"] - 1.0) <= 1e-12 and m["gross_pitch_error"] == 1.0


# ---- csrc/yin.hip on the host stand-in ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_yin_emu", os.path.join(gu.ROOT, "tests", "hip_emu", "build_yin_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("yin_emu"))))
    assert lib.t2amd_emulated() == 1
    for name, at in native._argtypes().items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = at, ctypes.c_int
    lib.t2amd_last_error.restype = ctypes.c_char_p
    return lib


@contextlib.contextmanager
def _emulated(lib):
    saved = (native._lib, native._validate_only)
    native._lib, native._validate_only = lib, True            # CPU pointers allowed, kernels DO run (emulated)
    try:
        yield
    finally:
        native._lib, native._validate_only = saved


def test_emulated_exact_periods(emu):
    with _emulated(emu):
        yc.periodic_structure(CPU)


def test_emulated_default_geometry_glides(emu):
    with _emulated(emu):
        yc.check_batch(yc.glide_signals(), CPU, yc.DEFAULT, "glides", min_decided=0.90)


@pytest.mark.parametrize("offset", range(4))
def test_emulated_small_geometry_at_every_alignment(emu, offset):
    with _emulated(emu):
        yc.check_batch(yc.small_signals(), CPU, yc.SMALL, "small+%d" % offset, offset=offset)


@pytest.mark.parametrize("name", ["ODD", "TAIL", "LONG"])
def test_emulated_other_geometries(emu, name):
    geo = getattr(yc, name)
    g = np.random.RandomState(5)
    n = 5 * geo["hop_length"] + 3
    signals = [yr.periodic(geo["frame_length"] // 4 - 3, n, 4), g.randn(n - geo["hop_length"]).astype(np.float32)]
    with _emulated(emu):
        yc.check_batch(signals, CPU, geo, name, offset=1)


def test_emulated_all_zero(emu):
    with _emulated(emu):
        yc.all_zero(CPU)
        yc.all_zero(CPU, yc.ODD)


def test_emulated_ragged_batch_equals_each_utterance_alone(emu):
    with _emulated(emu):
        yc.ragged_equals_alone(yc.small_signals(), CPU, yc.SMALL)


def test_emulated_module_equals_the_native_calls(emu):
    with _emulated(emu):
        yc.module_equals_native(yc.small_signals()[:5], CPU, yc.SMALL)


def test_refusals(emu):
    with _emulated(emu):
        yc.refusals(CPU)
        p = ctypes.c_void_p(torch.zeros(64).data_ptr())
        # the library's own checks, under the bindings'
        for args, word in (((p, 64, None, 1, 64, 5, 64, 16, 2, 32, 60.0, 0.1, p, p, p, None, None), b"W + tau_max + 1 exceeds"),
                           ((p, 64, None, 1, 64, 5, 64, 16, 1, 30, 60.0, 0.1, p, p, p, None, None), b"at least 2"),
                           ((p, 64, None, 1, 64, 5, 63, 16, 2, 30, 60.0, 0.1, p, p, p, None, None), b"even"),
                           ((p, 64, None, 1, 64, 4, 64, 16, 2, 30, 60.0, 0.1, p, p, p, None, None), b"T / hop_length + 1 frames"),
                           ((p, 32, None, 2, 64, 5, 64, 16, 2, 30, 60.0, 0.1, p, p, p, None, None), b"row stride")):
            assert emu.t2amd_yin_f32(*args) != 0 and word in emu.t2amd_last_error()


def test_host_tensors_are_refused():
    with pytest.raises(native.NativeError, match="no CPU path"):
        audio.yin(torch.zeros(1, 4000))


def test_f0_metrics():
    yc.check_metrics(CPU)
    with pytest.raises(ValueError, match="expected"):
        audio.f0_metrics(torch.zeros(2, 3), torch.zeros(2, 4), torch.zeros(2, 3), torch.zeros(2, 3))


# ---- the tool's wav mode: what needs no device -------------------------------------------------------------------------------
def test_evaluate_wavs_arguments(emu, tmp_path, capsys):
    da, db = tmp_path / "a", tmp_path / "b"
    da.mkdir()
    db.mkdir()
    for argv in (["--wavs", str(da)], ["--wavs", str(da), str(db), "--mels", str(da), str(db)],
                 ["--wavs", str(da), str(db), "--checkpoint", "x.pt"], ["--wavs", str(da), str(db), "--f0-min", "900"]):
        with pytest.raises(SystemExit):
            evaluate.main(argv)
    yc.write_wav(str(da / "u.wav"), yr.periodic(100, 3000), 22050)
    yc.write_wav(str(db / "u.wav"), yr.periodic(100, 3000), 16000)
    with pytest.raises(ValueError, match="sampling rate 16000, expected 22050"):
        evaluate.main(["--wavs", str(da), str(db), "--device", "cpu"])
    yc.write_wav(str(db / "u.wav"), np.stack([yr.periodic(100, 3000)] * 2, axis=1), 22050)
    with pytest.raises(ValueError, match="mono 16-bit"):
        evaluate.main(["--wavs", str(da), str(db), "--device", "cpu"])
    rows = [("a", 10, 10, 10, 1.0, 10.0, 0.5, 0.1, 0.0, 7), ("b", 10, 10, 10, 2.0, 30.0, float('nan'), 0.3, 0.2, 3),
            ("c", 10, 10, 10, 3.0, float('nan'), float('nan'), 1.0, float('nan'), 0)]
    assert evaluate.summarise_f0(rows) == {"f0_rmse_cents_mean": 20.0, "f0_rmse_cents_median": 20.0, "f0_corr_mean": 0.5,
                                           "vuv_error_mean": pytest.approx(1.4 / 3), "gross_pitch_error_mean": 0.1,
                                           "no_voiced_overlap": 1}
