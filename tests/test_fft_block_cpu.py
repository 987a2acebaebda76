"""The feed-forward Transformer block's convolutional feed-forward and add + LayerNorm without a GPU: the float64 definition
(tests/fft_block_ref.py) against float64 torch run on each utterance alone and against a padded batch (which differs), the float32
restatement against the float64 one, csrc/fft_block_rows.hip itself run on the host stand-in bit for bit against the restatement,
the refusals, and the C entries' argument checks (the MFMA entries in validate-only form)."""
import contextlib
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fft_block_cases as fc
import fft_block_ref as fr
import golden_util as gu
from tacotron2_amd import native, transformer

CPU = torch.device("cpu")
F32 = np.float32


# ---- the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 9])
@pytest.mark.parametrize("relu", [False, True])
def test_float64_definition_equals_torch_conv1d_on_each_utterance_alone(k, relu):
    """Every T_b from 1 to 9: forward and the autograd gradients of F.conv1d on the utterance trimmed to T_b."""
    batch = fc.conv_batch(tuple(range(1, 10)), 32, 64, k, relu, True, seed=k)
    w, b = torch.from_numpy(batch["w"]).double().requires_grad_(True), torch.from_numpy(batch["b"]).double().requires_grad_(True)
    for u in batch["utts"]:
        x = torch.from_numpy(u["x"]).double().requires_grad_(True)
        y = F.conv1d(x.t()[None], w, b, padding=k // 2)[0].t()
        y = F.relu(y) if relu else y
        dx, dw, db = torch.autograd.grad(y, (x, w, b), torch.from_numpy(u["g"]).double())
        for name, got in (("y", y.detach()), ("dx", dx), ("dw", dw), ("db", db)):
            assert np.abs(got.numpy() - u["f64"][name]).max() <= 1e-12 * max(1.0, np.abs(u["f64"][name]).max()), (u["T"], name)


def test_a_padded_batch_differs_in_the_last_frames_once_a_second_convolution_follows():
    """conv1 + ReLU + conv2 with k = 3 on a zero-padded batch: between the convolutions the hidden row T_b is ReLU(bias + the tap
    that still reaches frame T_b - 1), not zero, so the second convolution's last k // 2 frames differ from the utterance alone;
    every earlier frame agrees."""
    r = np.random.default_rng(3)
    w1, b1 = fc.conv_weights(32, 64, 3, True, 1)
    w2, b2 = fc.conv_weights(64, 32, 3, True, 2)
    T, Tm = 6, 9
    x = r.standard_normal((T, 32)).astype(F32)
    alone = fr.conv64(fr.conv64(x, w1, b1, True), w2, b2, False)
    xp = torch.zeros(Tm, 32, dtype=torch.float64)
    xp[:T] = torch.from_numpy(x).double()
    tw = lambda a: torch.from_numpy(a).double()                             # noqa: E731
    h = F.relu(F.conv1d(xp.t()[None], tw(w1), tw(b1), padding=1))
    padded = F.conv1d(h, tw(w2), tw(b2), padding=1)[0].t().numpy()
    assert np.abs(padded[:T - 1] - alone[:T - 1]).max() <= 1e-12
    assert np.abs(padded[T - 1] - alone[T - 1]).max() > 1e-3


@pytest.mark.parametrize("shape", [(32, 64, 3), (32, 160, 9), (96, 96, 5)])
def test_float32_restatement_is_close_to_float64(shape):
    """n = k Cin terms behind a value (B T behind dw): 8 n u max(1, |value|) bounds the restatement's error with room."""
    Cin, Cout, k = shape
    batch = fc.conv_batch((1, 5, 40), Cin, Cout, k, True, True)
    for u in batch["utts"]:
        for n, terms in (("y", k * Cin), ("dx", k * Cout)):
            assert fr.error(u["f32"][n], u["f64"][n]) <= 8 * terms * fr.U * max(1.0, np.abs(u["f64"][n]).max()), (u["T"], n)
    f64, f32 = fc.conv_batch_sums(batch, 40)
    for n in ("dw", "db"):
        assert fr.error(f32[n], f64[n]) <= 8 * 46 * fr.U * max(1.0, np.abs(f64[n]).max()), n
    ln = fc.ln_batch((3, 17), 384, True, plant=True)
    for u in ln["utts"]:
        # the planted row of |z| around 1e4: its mean carries u 1e4 of error, which the normalisation passes on to y
        assert fr.error(u["f32"]["y"], u["f64"]["y"]) <= 8 * fr.U * 1.0e4, u["T"]
        assert np.array_equal(u["f32"]["y"][0], ln["b"])                    # the all-equal row: var = 0, y = bias


# ---- csrc/fft_block_rows.hip on the host stand-in ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_fft_block_emu", os.path.join(gu.ROOT, "tests", "hip_emu", "build_fft_block_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("fft_block_emu"))))
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


@pytest.mark.parametrize("C", [32, 36, 384, 1028])
@pytest.mark.parametrize("residual", [False, True])
def test_emulated_add_layer_norm_equals_the_restatement_bit_for_bit(emu, C, residual):
    """Forward, dz, dweight and dbias through the autograd function, on a ragged batch with NaN in the padding."""
    batch = fc.ln_batch((0, 1, 3, 65), C, residual, plant=True)
    with _emulated(emu):
        out = fc.run_ln(batch, CPU, T=67, offset=1, device_lengths=False)
        fc.check_ln(batch, out, "emulated ", exact=True)
        again = fc.run_ln(batch, CPU, T=67, offset=0, device_lengths=False)
        for n in ("y", "dz", "dw", "db"):
            assert np.array_equal(fc.bits(out[n]), fc.bits(again[n])), n


def test_emulated_kept_rows_and_the_add_and_mask_form(emu):
    batch = fc.ln_batch((2, 5), 64, True)
    T, C = 6, 64
    with _emulated(emu):
        x, res = (fc.layout([u[n] for u in batch["utts"]], CPU, T) for n in ("x", "res"))
        lens = torch.tensor([2, 5], dtype=torch.int32)
        y, z = torch.full((2, T, C), 7.0), torch.full((2, T, C), 7.0)       # poisoned outputs
        mean, rstd = torch.full((2, T), 7.0), torch.full((2, T), 7.0)
        native.ffb_add_ln(x.contiguous(), res.contiguous(), torch.from_numpy(batch["w"]), torch.from_numpy(batch["b"]), lens, 1e-5, y, z, mean, rstd)
        for b, u in enumerate(batch["utts"]):
            for n, got in (("z", z), ("mean", mean), ("rstd", rstd), ("y", y)):
                assert np.array_equal(fc.bits(got[b, :u["T"]].numpy()), fc.bits(u["f32"][n])), (b, n)
                assert not fc.bits(got[b, u["T"]:].numpy()).any(), (b, n)
        xg, rg = x.clone().requires_grad_(True), res.clone().requires_grad_(True)
        s = transformer.add_layer_norm(xg, rg, None, None, [2, 5])
        g = fc.layout([u["g"] for u in batch["utts"]], CPU, T)
        s.backward(g)
        for b, u in enumerate(batch["utts"]):
            assert np.array_equal(fc.bits(s.detach()[b, :u["T"]].numpy()), fc.bits(u["x"] + u["res"]))
            assert not fc.bits(s.detach()[b, u["T"]:].numpy()).any()
            assert np.array_equal(fc.bits(xg.grad[b, :u["T"]].numpy()), fc.bits(u["g"])) and not fc.bits(xg.grad[b, u["T"]:].numpy()).any()
        assert torch.equal(xg.grad, rg.grad)
        with torch.no_grad():
            assert transformer.add_layer_norm(xg, rg, None, None, [2, 5]).grad_fn is None


def test_emulated_conv_rows_kernels_equal_the_restatement_bit_for_bit(emu):
    """The ReLU mask, the convolution's dbias, the transposed slab and the slice sum on a ragged batch of three slices."""
    Ts, T, C = (0, 1, 40, 33, 7, 40, 2, 40, 39, 40, 40, 17, 40, 40, 5, 40, 40, 40, 11, 40, 40, 40, 40, 3, 40, 40, 40, 40), 40, 32
    r = np.random.default_rng(5)
    gs = [r.standard_normal((t, C)).astype(F32) for t in Ts]
    ys = [r.standard_normal((t, C)).astype(F32) for t in Ts]
    B = len(Ts)
    Tp, S, L = fr.dw_plan(B, T)
    assert (Tp, S, L) == (64, 4, 448)
    with _emulated(emu):
        lens = torch.tensor(Ts, dtype=torch.int32)
        g, y = fc.layout(gs, CPU, T).contiguous(), fc.layout(ys, CPU, T).contiguous()
        gm = torch.full((B, T, C), 7.0)
        native.ffb_relu_mask(g, y, lens, gm)
        want = [fr.relu_mask32(a, b) for a, b in zip(gs, ys)]
        for b, t in enumerate(Ts):
            assert np.array_equal(fc.bits(gm[b, :t].numpy()), fc.bits(want[b])) and not fc.bits(gm[b, t:].numpy()).any(), b
        db = torch.full((C,), 7.0)
        ws = torch.zeros(native.fft_block_workspace(B, T, C, C, 1, 2), dtype=torch.uint8)
        native.ffb_colsum(g, None, None, None, lens, db, None, ws)
        assert np.array_equal(fc.bits(db.numpy()), fc.bits(fr.colsum32(gs, T)[0]))
        slab = torch.full((S, C, L), 7.0)
        assert emu.t2amd_ffb_transpose_f32(g.data_ptr(), lens.data_ptr(), B, T, C, slab.data_ptr(), slab.numel() * 4, None) == 0
        flat = np.zeros((S * L, C), F32)
        for b, a in enumerate(gs):
            flat[b * Tp:b * Tp + len(a)] = a
        assert np.array_equal(fc.bits(slab.numpy()), fc.bits(flat.reshape(S, L, C).transpose(0, 2, 1)))
        k, Cin, Cout = 3, 32, 64
        part = torch.from_numpy(r.standard_normal((S, k * Cin, Cout)).astype(F32))
        dw = torch.full((Cout, Cin, k), 7.0)
        assert emu.t2amd_ffb_dw_finish_f32(part.data_ptr(), S, Cin, Cout, k, dw.data_ptr(), None) == 0
        total = part[0].numpy()
        for s in range(1, S):
            total = total + part[s].numpy()
        assert np.array_equal(fc.bits(dw.numpy()), fc.bits(total.reshape(k, Cin, Cout).transpose(2, 1, 0)))
        assert native.fft_block_limits() == (4096, 4096, 9, 32, 65535)
        assert native.fft_block_workspace(B, T, Cin, Cout, k, 0) == 0
        assert native.fft_block_workspace(B, T, Cin, Cout, k, 1) == 4 * S * Cout * L + 4 * S * k * Cin * Cout
        P, _ = fr.sum_plan(B, T)
        assert native.fft_block_workspace(B, T, Cin, Cout, k, 2) == 4 * P * 2 * Cout


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(emu):
    conv, aln = transformer.ragged_conv1d, transformer.add_layer_norm
    with _emulated(emu):                                                    # host tensors pass the device check here
        x, w, b = torch.zeros(2, 6, 32), torch.zeros(64, 32, 3), torch.zeros(64)
        with pytest.raises(TypeError, match="ragged_conv1d: expected float32 x"):
            conv(x.double(), w, b)
        with pytest.raises(TypeError, match="ragged_conv1d: expected float32 weight"):
            conv(x, w.half(), b)
        with pytest.raises(TypeError, match="ragged_conv1d: expected float32 bias"):
            conv(x, w, b.double())
        with pytest.raises(ValueError, match=r"ragged_conv1d: expected x \(B, T, C\)"):
            conv(x[0], w, b)
        with pytest.raises(ValueError, match=r"ragged_conv1d: expected weight \(Cout, 32, k\)"):
            conv(x, torch.zeros(64, 64, 3), b)
        with pytest.raises(ValueError, match="ragged_conv1d: expected bias"):
            conv(x, w, torch.zeros(32))
        for k in (2, 11):
            with pytest.raises(ValueError, match="ragged_conv1d: a kernel width of %d is not odd and at most 9" % k):
                conv(x, torch.zeros(64, 32, k))
        with pytest.raises(ValueError, match="ragged_conv1d: 48 output channels are not a multiple of 32"):
            conv(x, torch.zeros(48, 32, 3))
        with pytest.raises(ValueError, match="ragged_conv1d: 16 input channels"):
            conv(torch.zeros(1, 4, 16), torch.zeros(32, 16, 3))
        with pytest.raises(ValueError, match="ragged_conv1d: 4128 output channels"):
            conv(x, torch.zeros(4128, 32, 1))
        with pytest.raises(ValueError, match="ragged_conv1d: 4097 frames exceed the limit of 4096"):
            conv(torch.zeros(1, 4097, 32), w)
        with pytest.raises(ValueError, match=r"ragged_conv1d: utterance 1: 7 frames do not lie in \[0, 6\]"):
            conv(x, w, b, [6, 7])
        with pytest.raises(ValueError, match="ragged_conv1d: 1 lengths for a batch of 2"):
            conv(x, w, b, [6])
        z = torch.zeros(2, 6, 64)
        with pytest.raises(TypeError, match="add_layer_norm: expected float32 x"):
            aln(z.double())
        with pytest.raises(TypeError, match="add_layer_norm: expected float32 residual"):
            aln(z, z.double())
        with pytest.raises(ValueError, match="add_layer_norm: expected residual"):
            aln(z, z[:1])
        for C in (16, 34, 4100):
            with pytest.raises(ValueError, match="add_layer_norm: %d channels are not a multiple of 4 from 32 to 4096" % C):
                aln(torch.zeros(1, 2, C))
        with pytest.raises(ValueError, match="add_layer_norm: weight and bias are given together"):
            aln(z, None, torch.zeros(64))
        with pytest.raises(ValueError, match="add_layer_norm: expected weight"):
            aln(z, None, torch.zeros(32), torch.zeros(64))
        for eps in (0.0, -1.0, float("nan"), "1", True):
            with pytest.raises(ValueError, match="add_layer_norm: eps must be a positive number"):
                aln(z, None, torch.zeros(64), torch.zeros(64), None, eps)
        with pytest.raises(ValueError, match=r"add_layer_norm: utterance 0: -1 frames do not lie in \[0, 6\]"):
            aln(z, None, None, None, [-1, 3])
    for bad in (2, (3, 2), (3, 3, 3), 11, True):
        with pytest.raises(ValueError, match="PositionwiseConvFF: kernel_size must be an odd int"):
            transformer.PositionwiseConvFF(64, 128, bad)
    with pytest.raises(ValueError, match="PositionwiseConvFF: d_inner must be a multiple of 32"):
        transformer.PositionwiseConvFF(64, 100, 3)
    with pytest.raises(ValueError, match="FFTransformer: n_layer must be a positive int"):
        transformer.FFTransformer(0, 2, 64, 32, 128, 3)
    ff = transformer.PositionwiseConvFF(64, 128, (9, 1), pre_lnorm=True)
    assert sorted(n for n, _ in ff.named_parameters()) == ["conv1.bias", "conv1.weight", "conv2.bias", "conv2.weight", "layer_norm.bias",
                                                           "layer_norm.weight"]
    assert tuple(ff.conv1.weight.shape) == (128, 64, 9) and tuple(ff.conv2.weight.shape) == (64, 128, 1)
    with pytest.raises(ValueError, match=r"PositionwiseConvFF: expected x \(B, T, 64\)"):
        ff(torch.zeros(2, 5, 32))
    net = transformer.FFTransformer(2, 2, 64, 32, 128, 3, n_embed=10)
    assert "layers.1.pos_ff.conv2.weight" in net.state_dict() and "layers.0.dec_attn.qkv_net.weight" in net.state_dict()
    assert tuple(net.word_emb.weight.shape) == (10, 64)
    with pytest.raises(ValueError, match=r"FFTransformer: expected integer symbols \(B, T\)"):
        net(torch.zeros(2, 5, 64))
    pe = transformer.positional_embedding(7, 64, torch.tensor([3, 7]))
    assert tuple(pe.shape) == (2, 7, 64) and not pe[0, 3:].any()
    assert torch.allclose(pe[1].double(), fc.pos_emb_ref(7, 64), atol=1e-5)


def test_host_tensors_are_refused():
    with pytest.raises(native.NativeError, match="ragged_conv1d: x is on cpu.*no CPU path"):
        transformer.ragged_conv1d(torch.zeros(1, 4, 32), torch.zeros(32, 32, 3))
    with pytest.raises(native.NativeError, match="add_layer_norm: x is on cpu.*no CPU path"):
        transformer.add_layer_norm(torch.zeros(1, 4, 32))
    with pytest.raises(native.NativeError, match="no CPU path"):
        transformer.PositionwiseConvFF(32, 64, 3)(torch.zeros(1, 4, 32))


# ---- the C entries' own checks -------------------------------------------------------------------------------------------------
def test_row_entries_refuse_bad_arguments(emu):
    base = torch.zeros(1 << 18).data_ptr() // 16 * 16 + 16
    at = lambda i: ctypes.c_void_p(base + i * (1 << 15))                    # noqa: E731
    x, res, w, b, y, z, mean, rstd, ws, g = (at(i) for i in range(10))
    n = ctypes.c_longlong(0)
    five = [ctypes.c_int(0) for _ in range(5)]
    assert emu.t2amd_fft_block_limits(*[ctypes.byref(v) for v in five]) == 0 and [v.value for v in five] == [4096, 4096, 9, 32, 65535]
    assert emu.t2amd_fft_block_limits(None, None, None, None, None) != 0 and b"fft_block: limits: null operand" in emu.t2amd_last_error()
    for args, word in (((1, 4, 32, 32, 3, 3), b"fft_block: workspace: which must be"), ((0, 4, 32, 32, 3, 0), b"at least 1 utterance"),
                       ((1, 4097, 32, 32, 3, 1), b"at most 4096 frames"), ((65536, 4, 32, 32, 3, 0), b"at most 65535 utterances"),
                       ((1, 4, 32, 32, 4, 0), b"an odd kernel width from 1 to 9"), ((1, 4, 32, 32, 11, 1), b"an odd kernel width"),
                       ((1, 4, 48, 32, 3, 0), b"input channels must be a multiple of 32"), ((1, 4, 32, 4128, 3, 0), b"output channels"),
                       ((1, 4, 32, 30, 3, 2), b"channels must be a multiple of 4")):
        assert emu.t2amd_fft_block_workspace(*args, ctypes.byref(n)) != 0 and word in emu.t2amd_last_error(), word
    assert emu.t2amd_fft_block_workspace(1, 4, 32, 32, 3, 0, None) != 0 and b"null operand" in emu.t2amd_last_error()
    names = ("x", "res", "w", "b", "len", "B", "T", "C", "eps", "y", "z", "mean", "rstd", "stream")
    ok = (x, res, w, b, None, 2, 4, 32, 1e-5, y, z, mean, rstd, None)
    ln = lambda **kw: emu.t2amd_ffb_add_ln_f32(*[kw.get(nm, d) for nm, d in zip(names, ok)])      # noqa: E731
    assert ln() == 0 and ln(res=None) == 0 and ln(w=None, b=None, mean=None, rstd=None) == 0 and ln(z=None, mean=None, rstd=None) == 0
    for kw, word in ((dict(x=None), b"fft_block: add_ln: null operand"), (dict(w=None), b"null operand"), (dict(mean=None), b"null operand"),
                     (dict(w=None, b=None), b"null operand"), (dict(C=30), b"channels must be a multiple of 4, from 32 to 4096"),
                     (dict(C=16), b"from 32 to 4096"), (dict(eps=0.0), b"eps must be positive"),
                     (dict(x=ctypes.c_void_p(x.value + 4)), b"aligned to 16 bytes"), (dict(y=x), b"must not overlap"),
                     (dict(z=res), b"must not overlap"), (dict(mean=rstd), b"must not overlap")):
        assert ln(**kw) != 0 and word in emu.t2amd_last_error(), word
    assert emu.t2amd_ffb_add_ln_bwd_f32(g, z, mean, rstd, w, None, 2, 4, 32, y, None) == 0
    for args, word in (((None, z, mean, rstd, w, None, 2, 4, 32, y, None), b"fft_block: add_ln_bwd: null operand"),
                       ((g, z, mean, rstd, w, None, 2, 4, 32, g, None), b"must not overlap"),
                       ((g, z, mean, rstd, w, None, 2, 4, 34, y, None), b"channels must be")):
        assert emu.t2amd_ffb_add_ln_bwd_f32(*args) != 0 and word in emu.t2amd_last_error(), word
    assert emu.t2amd_ffb_colsum_f32(g, None, None, None, None, 2, 4, 32, y, None, ws, 1024, None) == 0
    for args, word in (((g, None, None, None, None, 2, 4, 32, y, w, ws, 1024, None), b"fft_block: colsum: null operand"),
                       ((g, None, None, None, None, 2, 4, 32, y, None, ws, 100, None), b"workspace is smaller"),
                       ((g, None, None, None, None, 2, 4, 32, y, None, g, 1024, None), b"must not overlap")):
        assert emu.t2amd_ffb_colsum_f32(*args) != 0 and word in emu.t2amd_last_error(), word
    assert emu.t2amd_ffb_relu_mask_f32(g, y, None, 2, 4, 32, g, None) != 0 and b"fft_block: relu_mask: the output must not overlap" in emu.t2amd_last_error()
    assert emu.t2amd_ffb_transpose_f32(g, None, 2, 4, 32, ws, 100, None) != 0 and b"the slab is smaller" in emu.t2amd_last_error()
    assert emu.t2amd_ffb_dw_finish_f32(ws, 9, 32, 32, 3, y, None) != 0 and b"1 to 8 slices" in emu.t2amd_last_error()


def test_mfma_entries_refuse_bad_arguments_in_validate_only_form(native_lib):
    lib = native_lib
    base = torch.zeros(1 << 19).data_ptr() // 16 * 16 + 16
    at = lambda i: ctypes.c_void_p(base + i * (1 << 16))                    # noqa: E731
    x, img, bias, mask, y, g, dw, ws, ln = (at(i) for i in range(9))
    names = ("x", "xb", "xt", "img", "bias", "mask", "len", "B", "T", "Cin", "Cout", "k", "relu", "y", "stream")
    ok = (x, 256, 32, img, bias, mask, ln, 2, 8, 32, 64, 3, 1, y, None)
    dnames = ("g", "x", "xb", "xt", "len", "B", "T", "Cin", "Cout", "k", "dw", "ws", "ws_bytes", "stream")
    need = ctypes.c_longlong(0)
    native.set_validate_only(True)
    try:
        assert lib.t2amd_fft_block_workspace(2, 8, 32, 64, 3, 1, ctypes.byref(need)) == 0 and 0 < need.value <= 1 << 16
        dok = (g, x, 256, 32, ln, 2, 8, 32, 64, 3, dw, ws, need.value, None)
        conv = lambda **kw: lib.t2amd_ffb_conv_f32(*[kw.get(n, d) for n, d in zip(names, ok)])          # noqa: E731
        cdw = lambda **kw: lib.t2amd_ffb_conv_dw_f32(*[kw.get(n, d) for n, d in zip(dnames, dok)])      # noqa: E731
        assert conv() == 0 and conv(bias=None, mask=None, len=None) == 0 and conv(xt=36, xb=36 * 8) == 0
        for kw, word in ((dict(x=None), b"fft_block: conv: null operand"), (dict(y=None), b"fft_block: conv: null operand"),
                         (dict(img=None), b"null operand"), (dict(k=2), b"fft_block: conv: an odd kernel width from 1 to 9"),
                         (dict(Cin=48), b"input channels must be a multiple of 32"), (dict(Cout=4128), b"output channels must be"),
                         (dict(T=4097), b"at most 4096 frames"), (dict(B=65536), b"at most 65535 utterances"),
                         (dict(x=ctypes.c_void_p(x.value + 8)), b"x is not aligned to 16 bytes"), (dict(xt=34), b"x strides must be multiples of 4"),
                         (dict(xb=-256), b"x has a negative stride"), (dict(xt=16), b"x strides are shorter than a row"),
                         (dict(y=ctypes.c_void_p(y.value + 4)), b"must be aligned to 16 bytes"), (dict(y=x), b"must not overlap"),
                         (dict(y=img), b"must not overlap"), (dict(mask=y), b"must not overlap"), (dict(bias=y), b"must not overlap")):
            assert conv(**kw) != 0 and word in lib.t2amd_last_error(), word
        assert cdw() == 0 and cdw(len=None) == 0
        for kw, word in ((dict(g=None), b"fft_block: conv_dw: null operand"), (dict(dw=None), b"null operand"), (dict(ws=None), b"null operand"),
                         (dict(ws_bytes=need.value - 1), b"workspace is smaller"), (dict(k=10), b"fft_block: conv_dw: an odd kernel width"),
                         (dict(ws=ctypes.c_void_p(ws.value + 4)), b"must be aligned to 16 bytes"), (dict(dw=g), b"must not overlap"),
                         (dict(ws=x), b"must not overlap"), (dict(dw=ws), b"must not overlap"), (dict(xt=30), b"x strides must be multiples")):
            assert cdw(**kw) != 0 and word in lib.t2amd_last_error(), word
    finally:
        native.set_validate_only(False)


# ---- the rows file under the address and undefined-behaviour sanitizers --------------------------------------------------------
def test_rows_kernels_run_clean_in_a_stand_alone_sanitizer_program(tmp_path):
    """csrc/fft_block_rows.hip, the stand-in runtime and tests/hip_emu/fft_block_sanitize_main.cpp (its own main: every rows kernel
    once on a ragged batch with tensors of exactly the sizes the entries state) built by the host compiler with
    -fsanitize=address,undefined and run as a program of its own.  The MFMA file cannot be compiled for the host."""
    emu_dir = os.path.join(gu.ROOT, "tests", "hip_emu")
    exe = str(tmp_path / "fft_block_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-pthread", "-I", emu_dir, "-x", "c++",
                           os.path.join(gu.ROOT, "tacotron2_amd", "csrc", "fft_block_rows.hip"), os.path.join(emu_dir, "emu_runtime.cpp"),
                           os.path.join(emu_dir, "fft_block_sanitize_main.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
