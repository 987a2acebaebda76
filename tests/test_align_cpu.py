"""Forced alignment without a GPU: the two restatements (tests/align_ref.py) against brute-force enumeration and each other,
csrc/align.hip itself run on the host stand-in against them (tests/align_cases.py holds the cases the GPU file repeats),
alignment.alignment_metrics on hand-made matrices, the refusals, and the argument handling of the tools."""
import contextlib
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import align_cases as ac
import align_ref as ar
import golden_util as gu
from tacotron2_amd import alignment, native

CPU = torch.device("cpu")


# ---- the restatements ----------------------------------------------------------------------------------------------------------
def test_float64_restatement_equals_brute_force():
    g = np.random.RandomState(2)
    for T in range(1, 7):
        for N in range(1, T + 1):
            for kind in (ar.log_softmax_rows, ar.mixed_sign):
                x = kind(g, T, N)
                best, paths = ar.brute_force(x)
                s, dur, path = ar.align64(x)
                assert abs(s - best) <= 1e-12 * max(1.0, abs(best)), (T, N)
                assert any(np.array_equal(path, p) for p in paths) and ar.is_admissible(path, T, N)
                assert np.array_equal(dur, np.bincount(path, minlength=N))


def test_restatement_tie_rule_and_borders():
    s, dur, path = ar.align32(np.zeros((6, 3), np.float32))
    assert dur.tolist() == [1, 1, 4] and path.tolist() == [0, 1, 2, 2, 2, 2] and s == 0.0
    s, dur, path = ar.align32(np.arange(7 * 7, dtype=np.float32).reshape(7, 7))
    assert path.tolist() == list(range(7)) and s == sum(8.0 * i for i in range(7))
    # the walk ignores what is stored on the borders
    dur, path = ar._walk(np.ones((5, 2), bool), 5, 2)
    assert path.tolist() == [0, 0, 0, 0, 1]
    dur, path = ar._walk(np.zeros((3, 3), bool), 3, 3)
    assert path.tolist() == [0, 1, 2]


@pytest.mark.parametrize("kind", ac.KINDS)
def test_float32_restatement_is_optimal_within_the_bound(kind):
    for T, N in ac.SHAPES:
        x, (s32, _, p32), (s64, _, _) = ac.matrix(T, N, kind)
        returned, S = ar.path_score(x, p32)
        assert abs(returned - float(s64)) <= ar.bound(T, S) and abs(float(s32) - returned) <= ar.bound(T, S), (T, N)


# ---- csrc/align.hip on the host stand-in --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_align_emu", os.path.join(gu.ROOT, "tests", "hip_emu", "build_align_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("align_emu"))))
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


@pytest.mark.parametrize("kind", ac.KINDS)
@pytest.mark.parametrize("which", range(len(ac.SHAPES)))
def test_emulated_shapes(emu, which, kind):
    with _emulated(emu):
        ac.check_shape(*ac.SHAPES[which], kind, CPU)


def test_emulated_ties(emu):
    with _emulated(emu):
        ac.ties(CPU)


def test_emulated_planted_path(emu):
    with _emulated(emu):
        ac.planted(CPU)


def test_emulated_ragged_batch_equals_each_utterance_alone(emu):
    with _emulated(emu):
        ac.ragged_equals_alone(ac.ragged_mats(), CPU)


def test_emulated_module_equals_the_native_calls(emu):
    with _emulated(emu):
        ac.module_equals_native(ac.ragged_mats(), CPU)


def test_emulated_many_short_utterances(emu):
    with _emulated(emu):
        ac.many_short(CPU)


def test_emulated_attention_durations(emu):
    with _emulated(emu):
        ac.attention_case(CPU)


def test_emulated_tool_measure_skips_what_has_no_path(emu):
    """The tools' shared step: an utterance with fewer frames than tokens is left out, the others keep their own rows."""
    from tacotron2_amd import align
    A = torch.softmax(torch.randn(3, 9, 6, generator=torch.Generator().manual_seed(1)), dim=2)
    with _emulated(emu):
        keep, durs, metrics = align.measure(A, [6, 5, 2], [9, 4, 7])
        assert keep == [0, 2] and [d.tolist() for d in durs] == [alignment.attention_durations(A[b:b + 1], [ni], [no])[0][0, :ni].tolist()
                                                                  for b, ni, no in ((0, 6, 9), (2, 2, 7))]
        assert durs[0].sum() == 9 and durs[1].sum() == 7 and len(metrics) == 2 and len(metrics[0]) == 5
        assert align.measure(A, [6, 5], [5, 4]) == ([], [], [])


def test_emulated_walk_stays_inside_whatever_the_scores(emu):
    """Non-finite scores give an unspecified path, but an admissible one: the invariants of ``run`` hold."""
    g = np.random.RandomState(9)
    x = ar.mixed_sign(g, 40, 17)
    x[g.rand(40, 17) < 0.2] = np.nan
    x[g.rand(40, 17) < 0.2] = np.inf
    y = np.full((30, 30), -np.inf, np.float32)
    with _emulated(emu):
        ac.run([x, y], CPU)


def test_refusals(emu):
    with _emulated(emu):
        ac.refusals(CPU)
        p = ctypes.c_void_p(torch.zeros(4096).data_ptr())
        n = ctypes.c_longlong(0)
        # the library's own checks, under the bindings'
        for args, word in (((p, 40, 4, p, p, 1, 4097, 4, p, p, None, p, 1 << 20, None), b"at most 4096 frames"),
                           ((p, 4100, 1025, p, p, 1, 4, 1025, p, p, None, p, 1 << 20, None), b"at most 1024 tokens"),
                           ((p, 40, 4, p, p, 0, 10, 4, p, p, None, p, 1 << 20, None), b"1 to 2^20 utterances"),
                           ((p, 40, 3, p, p, 1, 10, 4, p, p, None, p, 1 << 20, None), b"score strides"),
                           ((p, 20, 4, p, p, 2, 10, 4, p, p, None, p, 1 << 20, None), b"score strides"),
                           ((p, 40, 4, p, p, 1, 10, 4, p, p, None, p, 10 * 4 + 15, None), b"workspace is smaller")):
            assert emu.t2amd_monotonic_align_f32(*args) != 0 and word in emu.t2amd_last_error(), word
        assert emu.t2amd_align_workspace(1, 0, 4, ctypes.byref(n)) != 0 and b"at least 1 frame" in emu.t2amd_last_error()
        assert emu.t2amd_align_workspace(3, 10, 5, ctypes.byref(n)) == 0 and n.value == 3 * 10 * 8 + 48


def test_host_tensors_are_refused():
    with pytest.raises(native.NativeError, match="no CPU path"):
        alignment.monotonic_align(torch.zeros(1, 4, 2))


# ---- alignment_metrics on hand-made matrices --------------------------------------------------------------------------------------
def test_metrics_one_hot_diagonal():
    A = np.zeros((1, 6, 3))
    path = np.array([[0, 0, 1, 1, 2, 2]])
    A[0, np.arange(6), path[0]] = 1.0
    m = alignment.alignment_metrics(A, path, [3], [6])
    assert {k: float(v[0]) for k, v in m.items()} == {"focus": 1.0, "path_mass": 1.0, "off_path": 0.0, "backward_steps": 0.0,
                                                      "max_duration": 2.0}
    # padding beyond the lengths is not looked at
    Ap = np.full((1, 8, 5), 9.0)
    Ap[0, :6, :3] = A[0]
    m = alignment.alignment_metrics(torch.from_numpy(Ap), torch.from_numpy(np.pad(path, ((0, 0), (0, 2)), constant_values=-1)), [3], [6])
    assert float(m["focus"][0]) == 1.0 and float(m["off_path"][0]) == 0.0 and float(m["max_duration"][0]) == 2.0


def test_metrics_one_backward_jump():
    A = np.full((1, 5, 4), 0.1)
    for t, n in enumerate([0, 1, 2, 1, 3]):                                 # frame 3 looks back at token 1
        A[0, t, n] = 0.7
    path = np.array([[0, 1, 2, 2, 3]])
    m = alignment.alignment_metrics(A, path, None, None)
    assert float(m["backward_steps"][0]) == 1.0 and float(m["off_path"][0]) == pytest.approx(0.2)
    assert float(m["focus"][0]) == pytest.approx(0.7) and float(m["path_mass"][0]) == pytest.approx((4 * 0.7 + 0.1) / 5)
    assert float(m["max_duration"][0]) == 2.0


def test_metrics_uniform_matrix():
    A = np.full((2, 8, 4), 0.25)
    path = np.array([[0, 1, 2, 3, 3, 3, 3, 3], [0, 0, 0, 1, 2, 3, -1, -1]])
    m = alignment.alignment_metrics(A, path, [4, 4], [8, 6])
    # the argmax is the lowest index among the maxima: token 0 on every frame
    assert m["focus"].tolist() == [0.25, 0.25] and m["path_mass"].tolist() == [0.25, 0.25] and m["backward_steps"].tolist() == [0, 0]
    assert m["off_path"].tolist() == [7 / 8, 3 / 6] and m["max_duration"].tolist() == [5, 3]
    with pytest.raises(ValueError, match="leaves its 4 tokens"):
        alignment.alignment_metrics(A, path, [4, 4], [8, 7])
    with pytest.raises(ValueError, match="expected"):
        alignment.alignment_metrics(A, path[:, :5], [4, 4], [8, 6])


# ---- the tools: what needs no device -----------------------------------------------------------------------------------------------
def test_tool_arguments_and_summary():
    from tacotron2_amd import align, evaluate
    for argv in ([], ["--checkpoint", "x.pt"], ["--checkpoint", "x.pt", "--filelist", "f"],
                 ["--checkpoint", "x.pt", "--filelist", "f", "-o", "d", "--batch", "0"]):
        with pytest.raises(SystemExit):
            align.main(argv)
    rows = [("a", 3, 10, 0.9, 0.8, 0.1, 0.0, 5.0), ("b", 4, 20, 0.7, 0.6, 0.3, 2.0, 9.0)]
    s = align.summarise(rows, ["c"])
    assert s == {"count": 2, "focus_mean": pytest.approx(0.8), "path_mass_mean": pytest.approx(0.7), "off_path_mean": pytest.approx(0.2),
                 "backward_steps_mean": 1.0, "max_duration_mean": 7.0, "unalignable": ["c"]}
    assert align.summarise([], [])["focus_mean"] is None
    with pytest.raises(SystemExit):
        evaluate.main(["--mels", "a", "b", "--alignment"])                  # the flag belongs to --checkpoint
