"""MCD-DTW without a GPU: the float64 restatement (tests/dtw_ref.py) against brute force and a closed form, csrc/dtw.hip itself run
on the host stand-in against the restatement (tests/dtw_cases.py holds the cases the GPU file repeats), the refusals, and the
evaluate tool's directory mode."""
import contextlib
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import dtw_cases as dc
import dtw_ref as dr
import golden_util as gu
from tacotron2_amd import audio, evaluate, native

CPU = torch.device("cpu")


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_restatement_optimum_equals_brute_force():
    g = np.random.RandomState(0)
    for n_a in range(1, 6):
        for n_b in range(1, 6):
            a, b = g.randn(n_a, 3), g.randn(n_b, 3)
            d = dr.cost_matrix(a, b)
            cost, steps, path = dr.dtw(a, b)
            assert abs(cost - dr.brute_force(d)) <= 1e-12 * max(cost, 1.0)
            assert dr.is_warping_path(path, n_a, n_b) and len(path) == steps
            assert abs(dr.path_cost(a, b, path) - cost) <= 1e-12 * max(cost, 1.0)
    # integer costs with many exact ties: still the optimum, and the path obeys the tie rule at every cell
    d = g.randint(0, 3, size=(5, 5)).astype(np.float64)
    D, N, ch = dr.accumulate(d)
    assert D[-1, -1] == dr.brute_force(d)
    for i in range(1, 5):
        for j in range(1, 5):
            cands = [D[i - 1, j - 1], D[i - 1, j], D[i, j - 1]]
            assert ch[i, j] == int(np.argmin(cands))             # argmin takes the first of equals: diagonal, up, left


def test_is_warping_path_rejects_what_is_not_one():
    assert dr.is_warping_path([(0, 0), (1, 1), (1, 2)], 2, 3)
    assert not dr.is_warping_path([(0, 0), (1, 2)], 2, 3)         # a jump
    assert not dr.is_warping_path([(0, 1), (1, 2)], 2, 3)         # wrong start
    assert not dr.is_warping_path([(0, 0), (1, 1)], 2, 3)         # wrong end
    assert not dr.is_warping_path([(0, 0), (0, 0), (1, 1), (1, 2)], 2, 3)   # a repeated cell


@pytest.mark.parametrize("n_mel,K", [(80, 13), (80, 32), (5, 1), (7, 6)])
def test_dct_is_the_orthonormal_dct2_without_c0(n_mel, K):
    M = dr.dct_matrix(n_mel, K)
    assert np.abs(M @ M.T - np.eye(K)).max() <= 1e-13               # orthonormal rows (K < n_mel)
    assert np.abs(M.sum(axis=1)).max() <= 1e-13                       # every row k >= 1 is orthogonal to the constant c0 row
    # the closed form of a cosine input: x_m = cos(pi q (m + 1/2) / N) has c_k = sqrt(N / 2) [k == q]
    q = min(K, 3)
    x = np.cos(np.pi * q * (np.arange(n_mel) + 0.5) / n_mel)
    want = np.zeros(K)
    want[q - 1] = np.sqrt(n_mel / 2.0)
    assert np.abs(dr.cepstrum(x[None, :, None], K)[0, 0] - want).max() <= 1e-12
    basis = audio.cepstral_basis(n_mel, K)
    assert basis.dtype == np.float32 and np.array_equal(basis, M.astype(np.float32))


# ---- csrc/dtw.hip on the host stand-in ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_dtw_emu", os.path.join(gu.ROOT, "tests", "hip_emu", "build_dtw_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("dtw_emu"))))
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


def test_band_width_is_a_multiple_of_the_wave(emu):
    with _emulated(emu):
        assert native.dtw_width() % 64 == 0 and 64 <= native.dtw_width() <= 1024


@pytest.mark.parametrize("K", dc.KS)
@pytest.mark.parametrize("which", range(9))
def test_emulated_optimum_and_path(emu, which, K):
    with _emulated(emu):
        n_a, n_b = dc.length_pairs()[which]
        dc.check_lengths(n_a, n_b, K, CPU)


def test_emulated_path_identity_where_the_optimum_is_unique_by_margin(emu):
    with _emulated(emu):
        assert dc.margin_seeds(CPU) >= 8


def test_emulated_exact_ties_follow_the_tie_rule(emu):
    with _emulated(emu):
        dc.tie_cases(CPU)


def test_emulated_ragged_batch_equals_each_pair_alone(emu):
    with _emulated(emu):
        dc.ragged_equals_alone(dc.ragged_pairs(), CPU)


def test_emulated_module_equals_the_native_calls(emu):
    with _emulated(emu):
        dc.module_equals_native(dc.ragged_pairs(K=5), CPU)


def test_emulated_cepstrum_against_the_restatement(emu):
    with _emulated(emu):
        errs = dc.cepstrum_errors(CPU, T=70, lengths=(70, 33, 1))
    for K, (e_k, e_t) in errs.items():
        print("FIGURE cepstrum K=%d: kernel max abs error %.3e, float32 torch.matmul %.3e" % (K, e_k, e_t))
        assert e_k <= 4 * e_t


def test_emulated_mcd_end_to_end(emu):
    ma, mb = dc.stretched_mels()
    with _emulated(emu):
        basis = torch.from_numpy(audio.cepstral_basis(80, 13))
        e_t = max(np.abs(torch.matmul(torch.from_numpy(m).transpose(1, 2), basis.t()).double().numpy() - dr.cepstrum(m)).max()
                  for m in (ma, mb))
        dc.mcd_end_to_end(CPU, 4 * e_t * np.sqrt(13.0))
        # a mel against itself: 0 dB along the diagonal
        mod = audio.MelCepstralDistortion(13, return_path=True)
        m = torch.from_numpy(ma)
        assert mod(m, m.clone()).item() == 0.0 and mod.last["steps"].item() == 120
        assert torch.equal(mod.last["path"][0, :120, 0], mod.last["path"][0, :120, 1])


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_host_tensors_are_refused():
    with pytest.raises(native.NativeError, match="no CPU path"):
        audio.dtw(torch.zeros(1, 3, 2), torch.zeros(1, 3, 2))
    with pytest.raises(native.NativeError, match="no CPU path"):
        audio.mel_cepstrum(torch.zeros(1, 80, 3))
    with pytest.raises(native.NativeError, match="no CPU path"):
        audio.MelCepstralDistortion()(torch.zeros(1, 80, 3), torch.zeros(1, 80, 4))


def test_refusals(emu):
    x, y = torch.zeros(2, 5, 4), torch.zeros(2, 6, 4)
    with _emulated(emu):
        for bad in ([0, 3], [5, 6]):
            with pytest.raises(ValueError, match="lengths must lie in"):
                audio.dtw(x, y, x_lengths=bad)
            with pytest.raises(ValueError, match="lengths must lie in"):
                audio.dtw(x, y, y_lengths=[6, 7] if bad[0] else [0, 1])
        with pytest.raises(ValueError, match="lengths for a batch"):
            audio.dtw(x, y, x_lengths=[5])
        long = torch.zeros(1, 4097, 1)
        with pytest.raises(ValueError, match=r"lengths must lie in \[1, 4096\]"):
            audio.dtw(long, torch.zeros(1, 3, 1))
        with pytest.raises(ValueError, match=r"lengths must lie in \[1, 4096\]"):
            audio.dtw(torch.zeros(1, 3, 1), long, y_lengths=[4097])
        cost, steps = audio.dtw(long, torch.zeros(1, 3, 1), x_lengths=[2])          # a long buffer with a short utterance is fine
        assert cost.item() == 0.0 and steps.item() == 3
        for K in (0, 33):
            with pytest.raises(ValueError, match="K must lie in|frames"):
                audio.dtw(torch.zeros(1, 3, K), torch.zeros(1, 3, K))
            with pytest.raises(ValueError, match="n_coef must lie in"):
                audio.mel_cepstrum(torch.zeros(1, 80, 3), n_coef=K)
            with pytest.raises(ValueError, match="n_coef must lie in"):
                audio.MelCepstralDistortion(K)
        with pytest.raises(ValueError, match=r"\(B, Tx, K\) and \(B, Ty, K\)"):
            audio.dtw(torch.zeros(1, 3, 4), torch.zeros(1, 3, 5))
        with pytest.raises(ValueError, match=r"\(B, Tx, K\) and \(B, Ty, K\)"):
            audio.dtw(torch.zeros(1, 3, 4), torch.zeros(2, 3, 4))
        with pytest.raises(ValueError, match="frames"):
            audio.dtw(torch.zeros(3, 4), torch.zeros(3, 4))
        with pytest.raises(TypeError, match="float32"):
            audio.dtw(x.double(), y.double())
        with pytest.raises(TypeError, match="float32"):
            audio.mel_cepstrum(torch.zeros(1, 80, 3, dtype=torch.float16))
        with pytest.raises(ValueError, match="log-mels"):
            audio.mel_cepstrum(torch.zeros(80, 3))
        with pytest.raises(ValueError, match="one B and n_mel"):
            audio.MelCepstralDistortion()(torch.zeros(1, 80, 3), torch.zeros(1, 40, 3))
        with pytest.raises(ValueError, match="lengths must lie in"):
            audio.MelCepstralDistortion()(torch.zeros(1, 80, 3), torch.zeros(1, 80, 3), len_a=[4])
        # the library's own checks, under the bindings'
        p = ctypes.c_void_p(x.data_ptr())
        for args, word in (((p, 20, p, 20, None, None, 1, 4097, 5, 4, p, p, None, 0, 0, None), b"4096"),
                           ((p, 20, p, 20, None, None, 1, 0, 5, 4, p, p, None, 0, 0, None), b"at least 1"),
                           ((p, 20, p, 20, None, None, 1, 5, 5, 33, p, p, None, 0, 0, None), b"1 to 32"),
                           ((p, 20, p, 20, None, None, 1, 5, 5, 0, p, p, None, 0, 0, None), b"1 to 32"),
                           ((p, 20, p, 20, None, None, 1, 5, 5, 4, p, p, p, 4, 5, None), b"smaller than")):
            assert emu.t2amd_dtw_f32(*args) != 0 and word in emu.t2amd_last_error()
        assert emu.t2amd_mel_cepstrum_f32(p, 240, 3, None, 1, 80, 3, p, 33, p, None) != 0 and b"1 to 32" in emu.t2amd_last_error()


# ---- the tool ----------------------------------------------------------------------------------------------------------------
def test_evaluate_directories(emu, tmp_path, capsys):
    ma, mb = dc.stretched_mels(n_mel=20, T=30)
    da, db = tmp_path / "a", tmp_path / "b"
    da.mkdir()
    db.mkdir()
    np.save(str(da / "same.npy"), ma[0])
    np.save(str(db / "same.npy"), ma[0])
    np.save(str(da / "other.npy"), ma[0])
    np.save(str(db / "other.npy"), mb[0])
    np.save(str(da / "only_a.npy"), ma[0])
    np.save(str(db / "only_b.npy"), mb[0])
    (db / "notes.txt").write_text("not a mel")
    out = tmp_path / "summary.json"
    with _emulated(emu):
        summary = evaluate.main(["--mels", str(da), str(db), "--n-coef", "5", "--batch", "1", "--device", "cpu", "-o", str(out)])
    lines = capsys.readouterr().out.strip().splitlines()
    assert json.loads(lines[-1]) == summary == json.loads(out.read_text())
    assert summary["count"] == 2 and summary["unmatched"] == ["only_a.npy", "only_b.npy"]
    assert "unmatched (only in A): only_a.npy" in lines and "unmatched (only in B): only_b.npy" in lines
    rows = dict((ln.split()[0], ln.split()[1:]) for ln in lines if ln.endswith(tuple("0123456789")) and ".npy " in ln)
    assert rows["same.npy"] == ["30", "30", "30", "0.0000"]
    fa, fb, steps, mcd_db = rows["other.npy"]
    assert (int(fa), int(fb)) == (30, mb.shape[2]) and max(30, mb.shape[2]) <= int(steps) <= 30 + mb.shape[2] - 1
    opt, ref_steps, _ = dr.dtw(dr.cepstrum(ma, 5)[0], dr.cepstrum(mb, 5)[0])
    assert abs(float(mcd_db) - dr.mcd(opt, ref_steps)) <= 1e-3 * dr.mcd(opt, ref_steps) + 1e-4
    assert summary["mcd_db_median"] == pytest.approx(float(mcd_db) / 2, abs=1e-4)
    assert summary["mcd_db_mean"] == pytest.approx(float(mcd_db) / 2, abs=1e-4) and summary["mcd_db_std"] > 0
    assert summary["length_ratio_mean"] == pytest.approx((1.0 + 30 / mb.shape[2]) / 2)
    with _emulated(emu):                                          # the batched call gives what the single calls gave
        again = evaluate.main(["--mels", str(da), str(db), "--n-coef", "5", "--device", "cpu"])
    assert again == summary
    with pytest.raises(SystemExit):
        evaluate.main([])
    with pytest.raises(SystemExit):
        evaluate.main(["--checkpoint", "x.pt"])
