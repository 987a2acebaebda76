"""The learned-aligner scores without a GPU: the float64 restatement (tests/aligner_ref.py) against central differences, the prior
against exact rational arithmetic, csrc/aligner_rows.hip itself run on the host stand-in through the cases the GPU file shares
(tests/aligner_cases.py), the refusals, and the C entries' argument checks."""
import contextlib
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import aligner_cases as ac
import aligner_ref as ar
import golden_util as gu
from tacotron2_amd import alignment, native

CPU = torch.device("cpu")


# ---- the restatements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 3), (3, 3, 2), (5, 2, 4), (9, 4, 5)])
def test_float64_gradients_equal_central_differences(shape):
    T, N, C = shape
    g = np.random.RandomState(T + 10 * N + 100 * C)
    q, k = g.randn(T, C).astype(np.float32), g.randn(N, C).astype(np.float32)
    logp, w, tau, h = ac.log_prior(g, T, N), g.randn(T, N), 0.7, 1e-5
    dq, dk, dlogp = ar.grads64(q, k, tau, w)

    def loss(q_, k_, lp_):
        z = -tau * ((np.asarray(q_, np.float64)[:, None, :] - np.asarray(k_, np.float64)[None, :, :]) ** 2).sum(axis=2)
        return float((w * (z - ar._lse64(z)[:, None] + lp_)).sum())

    for arr, grad, which in ((q, dq, 0), (k, dk, 1), (logp, dlogp, 2)):
        base = [np.asarray(a, np.float64) for a in (q, k, logp)]
        for idx in np.ndindex(arr.shape):
            up, dn = [a.copy() for a in base], [a.copy() for a in base]
            up[which][idx] += h
            dn[which][idx] -= h
            assert abs((loss(*up) - loss(*dn)) / (2 * h) - grad[idx]) <= 1e-7 * max(1.0, abs(grad[idx])), (shape, which, idx)


def test_float64_rows_are_an_attention_map_and_the_query_norm_term_vanishes():
    for T, N, C in ((1, 1, 1), (4, 3, 2), (9, 4, 5), (33, 70, 16)):
        c = ac.case(T, N, C, 1.0, True)
        assert np.abs(np.exp(c["f64"]["s"] - c["logp"]).sum(axis=1) - 1.0).max() <= 1e-12
        assert np.abs(c["f64"]["p"].sum(axis=1) - 1.0).max() <= 1e-12
        a, b = ar.grads64(c["q"], c["k"], 1.0, c["g"]), ar.grads64(c["q"], c["k"], 1.0, c["g"], keep_qnorm=True)
        assert np.abs(a[0] - b[0]).max() <= 1e-12 * max(1.0, np.abs(a[0]).max()) and np.array_equal(a[1], b[1])
        # the kernels' form of z differs from the definition by a constant along each row
        z_k = 2.0 * (c["q"].astype(np.float64) @ c["k"].astype(np.float64).T) - (c["k"].astype(np.float64) ** 2).sum(axis=1)[None, :]
        assert np.abs(ar._lse64(z_k) - c["f64"]["lse_k"]).max() <= 1e-9 * max(1.0, np.abs(c["f64"]["lse_k"]).max())
        # and the float32 restatement is close to the float64 one
        assert ar.error(c["f32"]["s"], c["f64"]["s"]) <= 64 * ar.U * max(1.0, np.abs(c["f64"]["z"]).max())


# ---- the prior -----------------------------------------------------------------------------------------------------------------
def test_prior_float64_equals_exact_rationals():
    for T in range(1, 13):
        for N in range(1, 9):
            exact, sums = ar.prior_exact(T, N)
            assert all(s == 1 for s in sums), (T, N)                        # every row sums to 1, exactly
            got = ar.prior64(T, N, 1.0)
            assert np.abs(got - exact).max() <= 1e-12, (T, N)
            if N == 1:
                assert not got.any()
    for scaling in (0.05, 0.5, 3.0):
        p = ar.prior64(37, 11, scaling)
        assert np.abs(np.exp(p).sum(axis=1) - 1.0).max() <= 1e-11


# ---- csrc/aligner_rows.hip on the host stand-in --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_aligner_emu", os.path.join(gu.ROOT, "tests", "hip_emu", "build_aligner_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("aligner_emu"))))
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


@pytest.mark.parametrize("with_prior", (False, True))
@pytest.mark.parametrize("which", range(len(ac.ROW_SHAPES)))
def test_emulated_row_kernels(emu, which, with_prior):
    T, N = ac.ROW_SHAPES[which]
    with _emulated(emu):
        mat = ac.row_mat(T, N)
        ac.check_rows(mat, ac.run_rows([mat], CPU, offset=(T + N) % 3, with_prior=with_prior), with_prior=with_prior)


def test_emulated_ragged_rows_equal_each_utterance_alone(emu):
    mats = [ac.row_mat(17, 65, 1), ac.row_mat(3, 1, 1), ac.row_mat(20, 9, 1), ac.row_mat(1, 1, 1)]
    with _emulated(emu):
        batch = ac.run_rows(mats, CPU, offset=1)
        for b, m in enumerate(mats):
            T, N = m[0].shape
            alone = ac.run_rows([m], CPU, offset=b % 3, pad=b)
            for name in ("s", "dlogp", "dz"):
                assert np.array_equal(ac.bits(batch[name][b, :T, :N]), ac.bits(alone[name][0, :T, :N])), (b, name)
            for name, n in (("lse", T), ("cs", N), ("kn", N)):
                assert np.array_equal(ac.bits(batch[name][b, :n]), ac.bits(alone[name][0, :n])), (b, name)
            ac.check_rows(m, batch, b)


def test_emulated_prior(emu):
    with _emulated(emu):
        for scaling in (1.0, 0.3):
            h = ac.check_prior(CPU, [(12, 8), (5, 1), (1, 1), (30, 30), (4, 9)], scaling, alignment.beta_binomial_log_prior)
        exact, _ = ar.prior_exact(12, 8)
        h = ac.check_prior(CPU, [(12, 8)], 1.0, alignment.beta_binomial_log_prior)
        assert np.abs(h[0, :12, :8] - exact).max() <= 4 * ar.U * max(1.0, np.abs(exact).max())
        a = alignment.beta_binomial_log_prior(torch.tensor([4, 2]), [3, 2])
        assert tuple(a.shape) == (2, 4, 3) and a.device.type == "cpu"


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(emu):
    with _emulated(emu):                                                    # host tensors pass the device check here
        q, k = torch.zeros(2, 6, 4), torch.zeros(2, 5, 4)
        f = alignment.aligner_scores
        with pytest.raises(TypeError, match="aligner_scores: expected float32 queries"):
            f(q.double(), k)
        with pytest.raises(TypeError, match="aligner_scores: expected float32 keys"):
            f(q, [[0.0]])
        with pytest.raises(TypeError, match="aligner_scores: expected float32 log_prior"):
            f(q, k, log_prior=torch.zeros(2, 6, 5, dtype=torch.float64))
        for bad_q, bad_k in ((torch.zeros(4), torch.zeros(4)), (q, torch.zeros(2, 5, 3)), (q, torch.zeros(3, 5, 4)), (q, k[0]),
                             (torch.zeros(2, 0, 4), k)):
            with pytest.raises(ValueError, match=r"aligner_scores: expected queries \(B, T, C\) or \(T, C\) and keys"):
                f(bad_q, bad_k)
        with pytest.raises(ValueError, match="aligner_scores: 513 channels exceed the limit of 512"):
            f(torch.zeros(1, 2, 513), torch.zeros(1, 2, 513))
        with pytest.raises(ValueError, match=r"aligner_scores: expected a log_prior of shape \(2, 6, 5\)"):
            f(q, k, log_prior=torch.zeros(2, 6, 4))
        for tau in (0.0, -1.0, float("inf"), float("nan"), "1"):
            with pytest.raises(ValueError, match="aligner_scores: the temperature must be a positive number"):
                f(q, k, temperature=tau)
        with pytest.raises(ValueError, match=r"aligner_scores: utterance 0: 0 frames and 1 tokens do not lie in \[1, 6\] and \[1, 5\]"):
            f(q, k, [0, 3], [1, 1])
        with pytest.raises(ValueError, match="aligner_scores: utterance 1: 3 frames and 6 tokens do not lie"):
            f(q, k, [6, 3], [5, 6])
        with pytest.raises(ValueError, match="aligner_scores: t_1 lengths for a batch of 2"):
            f(q, k, [6], [5, 5])
        with pytest.raises(ValueError, match="aligner_scores: 4097 frames and 2 tokens exceed the limits of 4096 frames and 1024"):
            f(torch.zeros(1, 4097, 2), torch.zeros(1, 2, 2))
        with pytest.raises(ValueError, match="aligner_scores: 3 frames and 1025 tokens exceed the limits"):
            f(torch.zeros(1, 3, 2), torch.zeros(1, 1025, 2))
        p = alignment.beta_binomial_log_prior
        with pytest.raises(ValueError, match=r"beta_binomial_log_prior: the scaling must lie in \(0, 1e6\]"):
            p([3], [2], scaling=0.0)
        with pytest.raises(ValueError, match="beta_binomial_log_prior: n_2 lengths for a batch of 1"):
            p([3], [2, 2])
        with pytest.raises(ValueError, match="beta_binomial_log_prior: utterance 0: 3 frames and 2 tokens do not lie"):
            p([3], [2], T=2)
        with pytest.raises(ValueError, match="beta_binomial_log_prior: expected the frames and tokens of at least one"):
            p([], [])
        with pytest.raises(ValueError, match="AlignerScores: the temperature"):
            alignment.AlignerScores(temperature=0)
        with pytest.raises(ValueError, match="AlignerScores: prior_scaling"):
            alignment.AlignerScores(prior_scaling=-1.0)
        assert not list(alignment.AlignerScores(prior_scaling=1.0).parameters())


def test_host_tensors_are_refused():
    with pytest.raises(native.NativeError, match="no CPU path"):
        alignment.aligner_scores(torch.zeros(1, 4, 2), torch.zeros(1, 3, 2))
    with pytest.raises(native.NativeError, match="no CPU path"):
        alignment.AlignerScores()(torch.zeros(4, 2), torch.zeros(3, 2))
    with pytest.raises(native.NativeError, match="no CPU path"):
        alignment.beta_binomial_log_prior([4], [2], device="cpu")


# ---- the C entries' own checks -------------------------------------------------------------------------------------------------
def test_row_entries_refuse_bad_arguments(emu):
    p = ctypes.c_void_p(torch.zeros(1 << 16).data_ptr() // 16 * 16 + 16)
    o = ctypes.c_void_p(p.value + (1 << 17))
    n = ctypes.c_longlong(0)
    for args, word in (((p, 40, 4, None, 0, 0, p, p, 1, 4097, 4, None, None), b"aligner_rows_fwd: at most 4096 frames"),
                       ((p, 40, 4, None, 0, 0, p, p, 1, 4, 1025, None, None), b"at most 1024 tokens"),
                       ((p, 40, 4, None, 0, 0, p, p, 0, 4, 4, None, None), b"1 to 65535 utterances"),
                       ((p, 40, 3, None, 0, 0, p, p, 1, 4, 4, None, None), b"score strides"),
                       ((p, 12, 4, None, 0, 0, p, p, 2, 4, 4, None, None), b"score strides"),
                       ((p, 40, 4, o, 40, 3, p, p, 1, 4, 4, None, None), b"prior strides"),
                       ((p, 40, 4, p, 40, 4, p, p, 1, 4, 4, None, None), b"must not overlap"),
                       ((None, 40, 4, None, 0, 0, p, p, 1, 4, 4, None, None), b"null operand")):
        assert emu.t2amd_aligner_rows_fwd_f32(*args) != 0 and word in emu.t2amd_last_error(), word
    far = [ctypes.c_void_p(p.value + i * (1 << 14)) for i in range(1, 6)]
    for args, word in (((p, 40, 3, p, p, 1, 4, 4, far[0], far[1], far[2], None, 0, 0, None), b"gradient strides"),
                       ((p, 40, 4, p, p, 1, 4, 4, far[0], far[1], far[2], far[3], 40, 3, None), b"prior gradient strides"),
                       ((p, 40, 4, p, p, 1, 4, 4, far[0], p, far[2], None, 0, 0, None), b"must not overlap"),
                       ((p, 40, 4, p, p, 1, 4, 4, None, far[1], far[2], None, 0, 0, None), b"null operand")):
        assert emu.t2amd_aligner_rows_bwd_f32(*args) != 0 and word in emu.t2amd_last_error(), word
    assert emu.t2amd_aligner_pack_keys_f32(p, p, 1, 4, 513, o, o, None) != 0 and b"1 to 512 channels" in emu.t2amd_last_error()
    assert emu.t2amd_aligner_pack_keys_f32(p, p, 1, 4, 4, ctypes.c_void_p(o.value + 4), o, None) != 0 and b"aligned" in emu.t2amd_last_error()
    assert emu.t2amd_aligner_transpose_f32(p, None, 1, 4, 4, o, None) != 0 and b"null operand" in emu.t2amd_last_error()
    assert emu.t2amd_beta_binomial_log_prior_f32(p, p, 1, 4, 4, 0.0, o, None) != 0 and b"scaling" in emu.t2amd_last_error()
    assert emu.t2amd_beta_binomial_log_prior_f32(p, p, 1, 0, 4, 1.0, o, None) != 0 and b"at least 1 frame" in emu.t2amd_last_error()
    assert emu.t2amd_aligner_workspace(1, 4, 4, 4, 3, ctypes.byref(n)) != 0 and b"which must be" in emu.t2amd_last_error()
    assert emu.t2amd_aligner_workspace(3, 10, 5, 80, 0, ctypes.byref(n)) == 0 and n.value == 4 * 3 * 5 * 96 + 4 * 16
    assert emu.t2amd_aligner_workspace(3, 10, 5, 80, 1, ctypes.byref(n)) == 0 and n.value == 4 * 3 * 5 * 96 + 4 * 16 + 4 * 32
    assert emu.t2amd_aligner_workspace(3, 10, 5, 80, 2, ctypes.byref(n)) == 0 \
        and n.value == 4 * 3 * 10 * 32 + 4 * 3 * 80 * 32 + 4 * 3 * 80 * 32 + 4 * 16


def test_score_entries_refuse_bad_arguments_in_validate_only_form(native_lib):
    lib = native_lib
    base = torch.zeros(1 << 16).data_ptr() // 16 * 16 + 16
    at = lambda i: ctypes.c_void_p(base + i * (1 << 13))                    # noqa: E731
    q, k, tl, nl, s, ws, g, dq, dk, kept = (at(i) for i in range(10))
    big = 1 << 13
    native.set_validate_only(True)
    try:
        fwd = lambda **kw: lib.t2amd_aligner_scores_f32(*[kw.get(n, d) for n, d in (                       # noqa: E731
            ("q", q), ("k", k), ("tl", tl), ("nl", nl), ("B", 1), ("T", 4), ("N", 4), ("C", 4), ("tau", 1.0), ("logp", None), ("pb", 0),
            ("pt", 0), ("s", s), ("sb", 16), ("st", 4), ("keep", 0), ("ws", ws), ("ws_bytes", big), ("stream", None))])
        assert fwd() == 0
        assert fwd(q=ctypes.c_void_p(q.value + 4), k=ctypes.c_void_p(k.value + 8)) == 0      # operands may start anywhere
        assert fwd(C=5, q=ctypes.c_void_p(q.value + 4)) == 0
        for kw, word in ((dict(C=513), b"aligner_scores: 1 to 512 channels"), (dict(T=4097), b"at most 4096 frames"),
                         (dict(tau=0.0), b"temperature must be positive"), (dict(q=None), b"null operand"), (dict(s=None), b"null operand"),
(dict(ws_bytes=4 * 4 * 32 + 15), b"workspace is smaller"),
                         (dict(keep=1, ws_bytes=4 * 4 * 32 + 16), b"workspace is smaller"), (dict(st=3), b"score strides"), (dict(s=q), b"must not overlap"),
                         (dict(ws=ctypes.c_void_p(ws.value + 8)), b"workspace is not aligned")):
            assert fwd(**kw) != 0 and word in lib.t2amd_last_error(), word
        bwd = lambda **kw: lib.t2amd_aligner_scores_bwd_f32(*[kw.get(n, d) for n, d in (                   # noqa: E731
            ("q", q), ("k", k), ("tl", tl), ("nl", nl), ("B", 1), ("T", 4), ("N", 4), ("C", 4), ("tau", 1.0), ("g", g), ("gb", 16), ("gt", 4),
            ("dq", dq), ("dk", dk), ("dlogp", None), ("db", 0), ("dt", 0), ("kept", kept), ("kept_bytes", big), ("ws", ws), ("ws_bytes", big),
            ("stream", None))])
        assert bwd() == 0
        for kw, word in ((dict(N=1025), b"aligner_scores_bwd: at most 1024 tokens"), (dict(g=None), b"null operand"),
                         (dict(kept_bytes=4 * 4 * 32 + 16), b"kept workspace"), (dict(ws_bytes=100), b"workspace is smaller"),
                         (dict(dq=q), b"must not overlap"), (dict(gt=3), b"gradient strides")):
            assert bwd(**kw) != 0 and word in lib.t2amd_last_error(), word
        prod = lambda which, **kw: lib.t2amd_aligner_product_f32(which, q, k, tl, nl, 1, 4, 4, 4, 1.0, kw.get("dq", dq), kw.get("dk", dk),     # noqa: E731
                                                                 kept, big, ws, kw.get("ws_bytes", big), None)
        assert prod(1, dq=None, dk=None) == 0 and prod(2, dk=None) == 0 and prod(3, dq=None) == 0
        for which, kw, word in ((0, {}, b"which must be 1"), (4, {}, b"which must be 1"), (2, dict(dq=None), b"null operand"),
                                (3, dict(dk=None), b"null operand"), (1, dict(ws_bytes=100), b"workspace is smaller")):
            assert prod(which, **kw) != 0 and word in lib.t2amd_last_error(), word
    finally:
        native.set_validate_only(False)
