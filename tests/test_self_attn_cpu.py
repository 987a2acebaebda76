"""The masked self-attention without a GPU: the float64 restatement (tests/self_attn_ref.py) against float64 torch autograd through
F.softmax, the float32 restatement against the float64 one, csrc/self_attn_rows.hip itself run on the host stand-in through the
cases the GPU file shares (tests/self_attn_cases.py), the refusals, and the C entries' argument checks (the MFMA entries in
validate-only form)."""
import contextlib
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import self_attn_cases as sc
import self_attn_ref as sr
from tacotron2_amd import native, transformer

CPU = torch.device("cpu")


# ---- the restatements ----------------------------------------------------------------------------------------------------------
def test_float64_restatement_equals_torch_autograd_through_softmax():
    """Every T from 1 to 9 at D = 32 as one ragged batch: the torch side masks the keys with -inf and the loss leaves the padded
    rows out."""
    H, D, Tm = 2, 32, 9
    cases = [sc.case(T, H, D, "normal", seed=1) for T in range(1, Tm + 1)]
    B = len(cases)
    pad = {n: torch.zeros(B, Tm, H, D, dtype=torch.float64) for n in ("q", "k", "v", "g")}
    for b, c in enumerate(cases):
        for n in pad:
            pad[n][b, :c["T"]] = torch.from_numpy(np.array(c[n])).double()
    q, k, v = (pad[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
    lens = torch.tensor([c["T"] for c in cases])
    dead = torch.arange(Tm)[None, :] >= lens[:, None]                       # (B, T)
    s = cases[0]["scale"] * torch.einsum("bthd,bjhd->bhtj", q, k)
    s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    o = torch.einsum("bhtj,bjhd->bthd", torch.nn.functional.softmax(s, dim=3), v)
    (o * pad["g"]).masked_fill(dead[:, :, None, None], 0.0).sum().backward()
    lse = torch.logsumexp(s, dim=3)
    for b, c in enumerate(cases):
        T, f = c["T"], c["f64"]
        for name, got in (("o", o.detach()[b, :T]), ("dq", q.grad[b, :T]), ("dk", k.grad[b, :T]), ("dv", v.grad[b, :T])):
            assert np.abs(got.numpy() - f[name]).max() <= 1e-12 * max(1.0, np.abs(f[name]).max()), (T, name)
        assert not any(np.abs(x.grad[b, T:].numpy()).any() for x in (q, k, v)), T
        assert np.abs(lse.detach()[b, :, :T].numpy() - f["lse"]).max() <= 1e-12 * max(1.0, np.abs(f["lse"]).max()), T
        assert np.abs(f["delta"] - np.einsum("thd,thd->ht", c["g"].astype(np.float64), f["o"])).max() <= 1e-12


@pytest.mark.parametrize("kind", sc.KINDS + sc.PLANTED)
def test_float32_restatement_is_close_to_float64_at_every_tile_width(kind):
    """The restatement's own error is rounding error: with n = T + D terms behind every value and a softmax whose argument's
    error the exponential multiplies by about |s|, 8 n u max(1, |s|) max(1, |value|) bounds it with room; the key-tile width
    changes the bits and not the size of the error."""
    T, H, D = (257, 1, 32) if kind in sc.PLANTED else (70, 2, 32)
    c = sc.case(T, H, D, kind)
    smax = max(1.0, max(np.abs(sr.forward64(c["q"][:, h], c["k"][:, h], c["v"][:, h], c["scale"])["s"]).max() for h in range(H)))
    for bn in (32, 64):
        f32 = c["f32"] if bn == 64 else sr.attention32(c["q"], c["k"], c["v"], c["g"], c["scale"], bn)
        for n in sc.TENSORS + ("delta",):
            vmax = max(1.0, np.abs(c["f64"][n]).max())
            assert sr.error(f32[n], c["f64"][n]) <= 8 * (T + D) * sr.U * smax * vmax, (kind, bn, n)
    if kind in sc.PLANTED:                                                  # the row of all-equal scores is a plain mean
        t1 = T // 2
        assert np.abs(c["f64"]["o"][t1, 0] - c["v"][:, 0].astype(np.float64).mean(axis=0)).max() <= 1e-12
        assert abs(c["f64"]["lse"][0, t1] - np.log(T)) <= 1e-12


# ---- csrc/self_attn_rows.hip on the host stand-in ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_self_attn_emu", os.path.join(gu.ROOT, "tests", "hip_emu", "build_self_attn_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("self_attn_emu"))))
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


@pytest.mark.parametrize("shape", [(1, 1, 32), (5, 2, 32), (33, 3, 32), (9, 2, 64), (7, 1, 96), (6, 2, 128)])
def test_emulated_delta_equals_the_restatement_bit_for_bit(emu, shape):
    T, H, D = shape
    cases = [sc.case(T, H, D, "normal", seed=2)]
    with _emulated(emu):
        sc.check_delta(cases, sc.run_delta(cases, CPU, offset=T % 3))


def test_emulated_ragged_delta_equals_each_utterance_alone(emu):
    cases = [sc.empty_case(2, 64)] + [sc.case(T, 2, 64, "normal", seed=2) for T in (1, 5, 9, 4)]
    with _emulated(emu):
        batch = sc.run_delta(cases, CPU, offset=1)
        sc.check_delta(cases, batch)
        for b, c in enumerate(cases[1:], 1):
            alone = sc.run_delta([c], CPU, offset=b % 3)
            assert np.array_equal(sc.bits(batch[b, :, :c["T"]]), sc.bits(alone[0]))
        assert native.self_attn_limits() == (4096, 16, 32, 128, 65535)
        assert native.self_attn_workspace(3, 10, 2, 32, 0) == 0
        assert native.self_attn_workspace(3, 10, 2, 32, 1) == native.self_attn_workspace(3, 10, 2, 32, 2) == 4 * 60
        assert native.self_attn_workspace(1, 3, 1, 64, 2) == 16


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(emu):
    f = transformer.self_attention
    with _emulated(emu):                                                    # host tensors pass the device check here
        q = torch.zeros(2, 6, 2, 32)
        with pytest.raises(TypeError, match="self_attention: expected float32 q"):
            f(q.double(), q, q)
        with pytest.raises(TypeError, match="self_attention: expected float32 v"):
            f(q, q, [[0.0]])
        with pytest.raises(TypeError, match="self_attention: expected float32 k"):
            f(q, q.half(), q)
        for bad in ((q, q[:1], q), (q, q, q[:, :5]), (torch.zeros(6, 32), torch.zeros(6, 32), torch.zeros(6, 32)), (q, q[0], q),
                    (torch.zeros(2, 0, 2, 32),) * 3):
            with pytest.raises(ValueError, match=r"self_attention: expected q, k and v of one shape \(B, T, H, D\) or \(T, H, D\)"):
                f(*bad)
        for D in (16, 48, 160):
            with pytest.raises(ValueError, match="self_attention: a head width of %d is not one of 32, 64, 96, 128" % D):
                f(*(torch.zeros(1, 2, 1, D),) * 3)
        with pytest.raises(ValueError, match="self_attention: 17 heads exceed the limit of 16"):
            f(*(torch.zeros(1, 2, 17, 32),) * 3)
        with pytest.raises(ValueError, match="self_attention: 4097 frames exceed the limit of 4096"):
            f(*(torch.zeros(1, 4097, 1, 32),) * 3)
        with pytest.raises(ValueError, match="self_attention: 4096 utterances times 16 heads exceed the limit of 65535"):
            f(*(torch.zeros(4096, 1, 16, 32),) * 3)
        for scale in (0.0, -1.0, float("inf"), float("nan"), "1", True):
            with pytest.raises(ValueError, match="self_attention: the scale must be a positive number"):
                f(q, q, q, scale=scale)
        with pytest.raises(ValueError, match=r"self_attention: utterance 1: 7 frames do not lie in \[0, 6\]"):
            f(q, q, q, [6, 7])
        with pytest.raises(ValueError, match=r"self_attention: utterance 0: -1 frames do not lie in \[0, 6\]"):
            f(q, q, q, [-1, 3])
        with pytest.raises(ValueError, match="self_attention: 1 lengths for a batch of 2"):
            f(q, q, q, [6])
    m = transformer.MultiHeadSelfAttention
    with pytest.raises(ValueError, match="MultiHeadSelfAttention: 17 heads exceed the limit of 16"):
        m(17, 64, 32)
    with pytest.raises(ValueError, match="MultiHeadSelfAttention: a head width of 40 is not one of"):
        m(2, 64, 40)
    with pytest.raises(ValueError, match="MultiHeadSelfAttention: d_model must be a positive int"):
        m(2, 0, 32)
    mod = m(2, 48, 32, pre_lnorm=True)
    assert sorted(n for n, _ in mod.named_parameters()) == ["layer_norm.bias", "layer_norm.weight", "o_net.weight", "qkv_net.bias",
                                                            "qkv_net.weight"]
    assert tuple(mod.qkv_net.weight.shape) == (192, 48) and tuple(mod.o_net.weight.shape) == (48, 64)
    with pytest.raises(ValueError, match=r"MultiHeadSelfAttention: expected x \(B, T, 48\)"):
        mod(torch.zeros(2, 5, 47))


def test_host_tensors_are_refused():
    q = torch.zeros(1, 4, 1, 32)
    with pytest.raises(native.NativeError, match="self_attention: q, k and v are on cpu.*no CPU path"):
        transformer.self_attention(q, q, q)
    with pytest.raises(native.NativeError, match="no CPU path"):
        transformer.MultiHeadSelfAttention(1, 32, 32)(torch.zeros(1, 4, 32))


# ---- the C entries' own checks -------------------------------------------------------------------------------------------------
def test_row_entries_refuse_bad_arguments(emu):
    p = ctypes.c_void_p(torch.zeros(1 << 16).data_ptr() // 16 * 16 + 16)
    o = ctypes.c_void_p(p.value + (1 << 16))
    d = ctypes.c_void_p(p.value + (1 << 17))
    n = ctypes.c_longlong(0)
    five = [ctypes.c_int(0) for _ in range(5)]
    assert emu.t2amd_self_attn_limits(*[ctypes.byref(x) for x in five]) == 0 and [x.value for x in five] == [4096, 16, 32, 128, 65535]
    assert emu.t2amd_self_attn_limits(None, None, None, None, None) != 0 and b"self_attn: limits: null operand" in emu.t2amd_last_error()
    for args, word in (((1, 4, 1, 32, 3), b"self_attn: workspace: which must be"), ((1, 4, 1, 32, -1), b"which must be"),
                       ((0, 4, 1, 32, 0), b"self_attn: workspace: at least 1 utterance and 1 frame"), ((1, 0, 1, 32, 0), b"at least 1"),
                       ((1, 4097, 1, 32, 0), b"at most 4096 frames"), ((1, 4, 0, 32, 0), b"1 to 16 heads"),
                       ((1, 4, 17, 32, 0), b"1 to 16 heads"), ((1, 4, 1, 16, 0), b"a head width of 32, 64, 96 or 128"),
                       ((1, 4, 1, 48, 0), b"a head width"), ((1, 4, 1, 160, 0), b"a head width"),
                       ((4096, 4, 16, 32, 0), b"at most 65535 utterances times heads")):
        assert emu.t2amd_self_attn_workspace(*args, ctypes.byref(n)) != 0 and word in emu.t2amd_last_error(), word
    assert emu.t2amd_self_attn_workspace(1, 4, 1, 32, 0, None) != 0 and b"null operand" in emu.t2amd_last_error()
    ok = (p, 256, 64, 32, o, None, 1, 4, 2, 32, d, None)
    assert emu.t2amd_self_attn_delta_f32(*ok) == 0

    def delta(**kw):
        names = ("g", "gb", "gt", "gh", "o", "len", "B", "T", "H", "D", "delta", "stream")
        return emu.t2amd_self_attn_delta_f32(*[kw.get(nm, dflt) for nm, dflt in zip(names, ok)])
    for kw, word in ((dict(g=None), b"self_attn: delta: null operand"), (dict(o=None), b"null operand"), (dict(delta=None), b"null operand"),
                     (dict(g=ctypes.c_void_p(p.value + 4)), b"the gradient is not aligned to 16 bytes"),
                     (dict(gt=66), b"the gradient strides must be multiples of 4 floats"), (dict(gh=-4), b"negative stride"),
                     (dict(D=40), b"a head width"), (dict(delta=p), b"must not overlap the inputs"),
                     (dict(delta=ctypes.c_void_p(o.value + 64)), b"must not overlap the inputs")):
        assert delta(**kw) != 0 and word in emu.t2amd_last_error(), word


def test_mfma_entries_refuse_bad_arguments_in_validate_only_form(native_lib):
    lib = native_lib
    base = torch.zeros(1 << 18).data_ptr() // 16 * 16 + 16
    at = lambda i: ctypes.c_void_p(base + i * (1 << 15))                    # noqa: E731
    q, k, v, o, lse, g, dq, dk, dv, ws, ln = (at(i) for i in range(11))
    fwd_names = ("q", "qb", "qt", "qh", "k", "kb", "kt", "kh", "v", "vb", "vt", "vh", "len", "B", "T", "H", "D", "scale", "o", "lse", "stream")
    fwd_ok = (q, 512, 64, 32, k, 512, 64, 32, v, 512, 64, 32, ln, 2, 8, 2, 32, 0.25, o, lse, None)
    bwd_names = fwd_names[:12] + ("o", "lse", "g", "gb", "gt", "gh", "len", "B", "T", "H", "D", "scale", "dq", "dk", "dv", "ws", "ws_bytes",
                                  "stream")
    bwd_ok = fwd_ok[:12] + (o, lse, g, 512, 64, 32, ln, 2, 8, 2, 32, 0.25, dq, dk, dv, ws, 128, None)
    native.set_validate_only(True)
    try:
        fwd = lambda **kw: lib.t2amd_self_attn_f32(*[kw.get(n, d) for n, d in zip(fwd_names, fwd_ok)])          # noqa: E731
        bwd = lambda **kw: lib.t2amd_self_attn_bwd_f32(*[kw.get(n, d) for n, d in zip(bwd_names, bwd_ok)])      # noqa: E731
        assert fwd() == 0 and fwd(lse=None) == 0 and fwd(len=None) == 0
        # the three chunks of one packed projection: interleaved inputs are no overlap
        assert fwd(k=ctypes.c_void_p(q.value + 256), v=ctypes.c_void_p(q.value + 512), qb=1536, qt=192, kb=1536, kt=192, vb=1536, vt=192) == 0
        for kw, word in ((dict(q=None), b"self_attn: forward: null operand"), (dict(o=None), b"self_attn: forward: null operand"),
                         (dict(D=48), b"self_attn: forward: a head width of 32, 64, 96 or 128"), (dict(H=17), b"1 to 16 heads"),
                         (dict(T=4097), b"at most 4096 frames"), (dict(B=40000), b"at most 65535 utterances times heads"),
                         (dict(k=ctypes.c_void_p(k.value + 8)), b"k is not aligned to 16 bytes"), (dict(vt=66), b"v strides must be multiples of 4"),
                         (dict(qb=-512), b"q has a negative stride"), (dict(scale=0.0), b"the scale must be positive and finite"),
                         (dict(scale=float("nan")), b"the scale must be positive"), (dict(o=ctypes.c_void_p(o.value + 4)), b"o is not aligned"),
                         (dict(o=q), b"must not overlap"), (dict(lse=k), b"must not overlap"), (dict(lse=o), b"must not overlap")):
            assert fwd(**kw) != 0 and word in lib.t2amd_last_error(), word
        assert bwd() == 0 and bwd(len=None) == 0
        for kw, word in ((dict(g=None), b"self_attn: backward: null operand"), (dict(lse=None), b"self_attn: backward: null operand"),
                         (dict(dk=None), b"null operand"), (dict(ws=None), b"null operand"), (dict(ws_bytes=127), b"workspace is smaller"),
                         (dict(gt=66), b"the gradient strides must be multiples of 4"), (dict(D=16), b"self_attn: backward: a head width"),
                         (dict(dq=ctypes.c_void_p(dq.value + 4)), b"must be aligned to 16 bytes"), (dict(dq=q), b"must not overlap"),
                         (dict(dv=dk), b"must not overlap"), (dict(dk=g), b"must not overlap"), (dict(ws=lse), b"must not overlap"),
                         (dict(dv=o), b"must not overlap"), (dict(scale=-1.0), b"the scale must be positive")):
            assert bwd(**kw) != 0 and word in lib.t2amd_last_error(), word
    finally:
        native.set_validate_only(False)
