"""The forward-sum alignment likelihood without a GPU: the float64 restatement (tests/forward_sum_ref.py) against brute-force
enumeration, against float64 ``F.ctc_loss`` with a blank that can never be taken and against central differences; the float32
restatement of the kernel's normalisation against it; csrc/forward_sum.hip itself run on the host stand-in through the cases the
GPU file repeats (tests/forward_sum_cases.py); the refusals; and the argument handling of the tools."""
import contextlib
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import align_ref as ar
import forward_sum_cases as fc
import forward_sum_ref as fr
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
                want_z, want_g = fr.brute_force(x)
                z, gamma, soft = fr.forward_sum64(x)
                assert abs(z - want_z) <= 1e-12 * max(1.0, abs(want_z)), (T, N)
                assert np.abs(gamma - want_g).max() <= 1e-12 and np.abs(soft - want_g.sum(axis=0)).max() <= 1e-12, (T, N)
                assert not gamma[~fr.in_band(T, N)].any()
    x = ar.mixed_sign(g, 6, 3)
    x[:, 1] = -np.inf
    assert fr.brute_force(x)[0] == -np.inf and fr.forward_sum64(x)[0] == -np.inf and not fr.forward_sum64(x)[1].any()


def ctc_neg_log_z(x):
    """float64 F.ctc_loss of the scores with a blank column of -inf in front and the targets 1 .. N: -log Z."""
    T, N = x.shape
    lp = torch.cat([torch.full((T, 1), -np.inf, dtype=torch.float64), torch.from_numpy(np.asarray(x, dtype=np.float64))], dim=1)
    return torch.nn.functional.ctc_loss(lp.unsqueeze(1), torch.arange(1, N + 1).unsqueeze(0), torch.tensor([T]), torch.tensor([N]),
                                        blank=0, reduction='none')


def test_float64_restatement_equals_ctc_loss_with_an_impossible_blank():
    for T, N in ((1, 1), (2, 2), (9, 1), (7, 7), (65, 64), (130, 63), (259, 256), (4096, 5)):
        for kind in fc.KINDS:
            x, _, (z, _, _) = fc.matrix(T, N, kind)
            got = float(ctc_neg_log_z(x)[0])
            assert abs(got + z) <= 1e-12 * max(1.0, abs(z)), (T, N, kind, got, z)


def test_gamma_is_the_derivative_of_log_z():
    g = np.random.RandomState(4)
    h = 1e-4
    for T, N in ((1, 1), (4, 2), (6, 6), (9, 4), (12, 5)):
        x = ar.mixed_sign(g, T, N)
        _, gamma, _ = fr.forward_sum64(x)

        def log_z(t, n, d):                                                # the float32 step taken is the step measured
            y = x.copy()
            y[t, n] = np.float32(y[t, n] + d)
            return fr.forward_sum64(y)[0], float(y[t, n])

        for t in range(T):
            for n in range(N):
                (zp, vp), (zm, vm) = log_z(t, n, h), log_z(t, n, -h)
                assert abs((zp - zm) / (vp - vm) - gamma[t, n]) <= 1e-6, (T, N, t, n)


@pytest.mark.parametrize("kind", fc.KINDS)
def test_gamma_rows_sum_to_one_and_durations_to_the_frames(kind):
    for T, N in fc.SHAPES:
        x, (z32, g32, d32), (z64, g64, d64) = fc.matrix(T, N, kind)
        assert np.abs(g64.sum(axis=1) - 1.0).max() <= 1e-9 and abs(d64.sum() - T) <= 1e-9 * T, (T, N)
        assert not g64[~fr.in_band(T, N)].any() and not g32[~fr.in_band(T, N)].any()
        assert ar.align64(x)[0] <= z64 + 1e-9 * max(1.0, abs(z64))          # the best path is one of the paths summed
        # the normalised float32 scheme: a row's maximum is one score away from its offset, so each of the T rounded adds and
        # subtractions on the way to log Z errs by at most 2^-24 max|l|, and the last rounding by 2^-24 |log Z|; gamma within
        # 1e-2 even at 1030 x 1024 (the plain float32 form misses that at 1030 x 1024 and at 4096 x 5)
        assert abs(float(z32) - z64) <= fr.U * (4 * T * float(np.abs(x).max()) + 8 * max(1.0, abs(z64))), (T, N)
        assert np.abs(g32 - g64).max() <= 1e-2, (T, N)


# ---- csrc/forward_sum.hip on the host stand-in ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_forward_sum_emu",
                                                  os.path.join(gu.ROOT, "tests", "hip_emu", "build_forward_sum_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("forward_sum_emu"))))
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


@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("which", range(len(fc.SHAPES)))
def test_emulated_shapes(emu, which, kind):
    with _emulated(emu):
        fc.check_shape(*fc.SHAPES[which], kind, CPU)


def test_emulated_ragged_batch_equals_each_utterance_alone(emu):
    with _emulated(emu):
        fc.ragged_equals_alone(fc.ragged_mats(), CPU)


def test_emulated_module_equals_the_native_calls_and_autograd(emu):
    with _emulated(emu):
        fc.module_equals_native(fc.ragged_mats(), CPU)
        fc.loss_module(fc.ragged_mats(), CPU)


def test_emulated_many_short_utterances(emu):
    with _emulated(emu):
        fc.many_short(CPU)


def test_emulated_planted_path_and_all_zero_scores(emu):
    with _emulated(emu):
        fc.planted(CPU)
        fc.all_zero(CPU)


def test_emulated_impossible_cells(emu):
    with _emulated(emu):
        fc.impossible(CPU)


def test_emulated_non_finite_scores_leave_the_poison_intact(emu):
    with _emulated(emu):
        fc.non_finite(CPU)


def test_refusals(emu):
    with _emulated(emu):
        fc.refusals(CPU)
        p = ctypes.c_void_p(torch.zeros(1 << 20).data_ptr() // 16 * 16 + 16)
        n = ctypes.c_longlong(0)
        big = 1 << 21
        # the library's own checks, under the bindings'
        for args, word in (((p, 40, 4, p, p, 1, 4097, 4, p, 0, p, big, None), b"forward_sum: at most 4096 frames"),
                           ((p, 4100, 1025, p, p, 1, 4, 1025, p, 0, p, big, None), b"at most 1024 tokens"),
                           ((p, 40, 4, p, p, 0, 10, 4, p, 0, p, big, None), b"1 to 2^20 utterances"),
                           ((p, 40, 3, p, p, 1, 10, 4, p, 0, p, big, None), b"score strides"),
                           ((p, 20, 4, p, p, 2, 10, 4, p, 0, p, big, None), b"score strides"),
                           ((p, 40, 4, p, p, 1, 10, 4, p, 0, p, 15, None), b"workspace is smaller"),
                           ((p, 40, 4, p, p, 1, 10, 4, p, 1, p, 10 * 4 * 4 + 10 * 8 + 15, None), b"workspace is smaller"),
                           ((p, 40, 4, p, p, 1, 10, 4, None, 0, p, big, None), b"null operand")):
            assert emu.t2amd_forward_sum_f32(*args) != 0 and word in emu.t2amd_last_error(), word
        for args, word in (((p, 40, 4, p, p, 1, 10, 4, p, None, p, 40, 3, None, p, big, None), b"gradient strides"),
                           ((p, 40, 4, p, p, 1, 10, 4, p, None, p, 40, 4, None, p, 10 * 4 * 4 + 10 * 8 + 15, None), b"workspace is smaller"),
                           ((p, 40, 4, p, p, 1, 10, 4, p, None, None, 40, 4, None, p, big, None), b"null operand")):
            assert emu.t2amd_forward_sum_bwd_f32(*args) != 0 and word in emu.t2amd_last_error(), word
        assert emu.t2amd_forward_sum_workspace(1, 0, 4, 1, ctypes.byref(n)) != 0 and b"at least 1 frame" in emu.t2amd_last_error()
        assert emu.t2amd_forward_sum_workspace(3, 10, 5, 1, ctypes.byref(n)) == 0 and n.value == 3 * 10 * 8 * 4 + 3 * 10 * 8 + 48
        assert emu.t2amd_forward_sum_workspace(3, 10, 5, 0, ctypes.byref(n)) == 0 and n.value == 48


def test_host_tensors_are_refused():
    for fn in (alignment.forward_sum, alignment.alignment_posterior, alignment.ForwardSumLoss()):
        with pytest.raises(native.NativeError, match="no CPU path"):
            fn(torch.zeros(1, 4, 2))


# ---- the tools: what needs no device -----------------------------------------------------------------------------------------------
def test_tool_arguments_and_summary():
    from tacotron2_amd import align, evaluate
    rows = [("a", 3, 10, 0.9, 0.8, 0.1, 0.0, 5.0), ("b", 4, 20, 0.7, 0.6, 0.3, 2.0, 9.0)]
    plain = align.summarise(rows, ["c"])
    assert "log_likelihood_per_frame_mean" not in plain and len(plain) == 7        # what it is without the flag
    s = align.summarise(rows, ["c"], [(-1.5, -0.25), (-2.5, -0.75)])
    assert {k: s[k] for k in plain} == plain
    assert set(s) - set(plain) == {"log_likelihood_per_frame_mean", "path_log_posterior_per_frame_mean"}
    assert s["log_likelihood_per_frame_mean"] == pytest.approx(-2.0) and s["path_log_posterior_per_frame_mean"] == pytest.approx(-0.5)
    assert align.summarise([], [], [])["log_likelihood_per_frame_mean"] is None
    with pytest.raises(SystemExit):
        align.main(["--posterior"])                                         # the required arguments are still required
    with pytest.raises(SystemExit):
        evaluate.main(["--mels", "a", "b", "--posterior"])                  # the flag belongs to --checkpoint --alignment
    with pytest.raises(SystemExit):
        evaluate.main(["--checkpoint", "x.pt", "--filelist", "f", "--posterior"])


def test_emulated_tool_posterior_of_a_batch(emu):
    """The tools' shared step: soft durations that sum to the frames, log Z per frame, and the path's log posterior <= 0."""
    from tacotron2_amd import align
    A = torch.softmax(torch.randn(3, 9, 6, generator=torch.Generator().manual_seed(1)), dim=2)
    ni, no = [6, 2], [9, 7]
    scores = torch.tensor([-3.0, -1.0])
    with _emulated(emu):
        soft, post = align.posterior(A[[0, 2]], ni, no, scores)
    assert len(soft) == 2 and soft[0].shape == (6,) and soft[1].shape == (2,) and soft[0].dtype == np.float32
    assert abs(soft[0].sum() - 9) <= 9e-3 and abs(soft[1].sum() - 7) <= 7e-3
    for j in range(2):
        x = np.log(np.maximum(A[[0, 2][j], :no[j], :ni[j]].numpy(), 1e-8)).astype(np.float32)
        z = fr.forward_sum64(x)[0]
        assert post[j][0] == pytest.approx(z / no[j], abs=1e-5) and post[j][1] == pytest.approx((float(scores[j]) - z) / no[j], abs=1e-5)
