"""WaveGlow without a GPU: weight-norm folding, the shape-derived configuration and its refusals, the layout identities
of the native path (upsample phases, grouped rows, gate packing) in float64, the argument checks of the new entry points
(validate-only), and csrc/waveglow.hip's flow tail run on the host stand-in of tests/hip_emu -- directly against float64
numpy on a ragged batch, and as part of the whole WaveGlow.infer with the two products stood in by float64 torch,
against the restatement tests/waveglow_ref.py."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import waveglow_ref as wr
from tacotron2_amd import native
from tacotron2_amd import waveglow as wgm

EMU = os.path.join(gu.ROOT, "tests", "hip_emu")
SMALL = dict(C=64, L=2, n_flows=4, n_group=8, n_early_every=2, n_early_size=2)


def _small_ref(seed=0, weight_norm=True):
    return wr.make_ref(seed=seed, weight_norm=weight_norm, **SMALL).double()


def test_weight_norm_folding_is_bit_equal_to_remove_weight_norm():
    m = _small_ref()
    sd = {k: v.float() for k, v in m.state_dict().items()}
    assert any(k.endswith('weight_g') for k in sd)
    folded = wgm.fold_weight_norm(sd)
    want = wr.folded_state_dict(m.float())
    assert set(folded) == set(want)
    for k in want:
        assert torch.equal(folded[k], want[k]), k


def test_config_from_shapes_and_refusals():
    cfg = wgm.config_from_state_dict(_small_ref().state_dict())
    assert cfg == dict(n_mel_channels=80, n_flows=4, n_group=8, n_early_every=2, n_early_size=2,
                       WN_config=dict(n_layers=2, n_channels=64, kernel_size=3))
    pub = wgm.WaveGlow(80, 12, 8, 4, 2, dict(n_layers=8, n_channels=256, kernel_size=3))
    assert wgm.config_from_state_dict(pub.state_dict()) == dict(
        n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2,
        WN_config=dict(n_layers=8, n_channels=256, kernel_size=3))
    assert pub.flow_channels == [8] * 4 + [6] * 4 + [4] * 4 and pub.n_remaining_channels == 4
    assert [s[1] for s in pub.noise_shapes(2, 10)] == [4, 2, 2]
    with pytest.raises(ValueError, match="kernel_size"):
        wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=5))
    with pytest.raises(ValueError, match="even"):
        wgm.WaveGlow(80, 4, 7, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=3))
    with pytest.raises(ValueError, match="multiple of 64"):
        wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=96, kernel_size=3))
    legacy = dict(_small_ref().state_dict())
    legacy['WN.0.cond_layers.0.weight'] = torch.zeros(1)
    with pytest.raises(ValueError, match="convert_model.py"):
        wgm.config_from_state_dict(legacy)
    with pytest.raises(ValueError, match="geometry"):
        wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=3, n_channels=64, kernel_size=3)).load_state_dict(
            _small_ref().state_dict())


def test_upsample_phase_formulation_equals_conv_transpose_and_trim():
    g = torch.Generator().manual_seed(3)
    nm, N = 16, 5
    W = torch.randn(nm, nm, 1024, generator=g, dtype=torch.float64)
    bias = torch.randn(nm, generator=g, dtype=torch.float64)
    x = torch.randn(1, nm, N, generator=g, dtype=torch.float64)
    ref = F.conv_transpose1d(x, W, bias, stride=256)[:, :, :-768]
    up_w = W.view(nm, nm, 4, 256).permute(3, 1, 2, 0).reshape(256 * nm, 4 * nm)
    xt = x[0].t()                                                        # [q][ci]
    A = torch.cat([torch.cat([torch.zeros(j, nm, dtype=torch.float64), xt[:N - j]], 0) for j in range(4)], 1)
    out = A @ up_w.t() + bias.repeat(256)                                # [q][p n_mel + co]
    assert torch.allclose(out.view(N, 256, nm).permute(2, 0, 1).reshape(nm, 256 * N), ref[0], rtol=0, atol=1e-12)


def test_grouped_rows_and_permuted_cond_columns_equal_unfold_path():
    g = torch.Generator().manual_seed(4)
    nm, G, T, Co = 16, 8, 64, 24
    y = torch.randn(1, nm, T, generator=g, dtype=torch.float64)
    Wc = torch.randn(Co, nm * G, 1, generator=g, dtype=torch.float64)
    s = y.unfold(2, G, G).permute(0, 2, 1, 3).contiguous().view(1, T // G, -1).permute(0, 2, 1)
    ref = F.conv1d(s, Wc)[0].t()                                         # [R][Co]
    rows = y[0].t().reshape(T // G, G * nm)                              # sample-major: column g n_mel + c
    Wp = Wc.view(Co, nm, G).permute(0, 2, 1).reshape(Co, G * nm)
    assert torch.allclose(rows @ Wp.t(), ref, rtol=0, atol=1e-12)


def test_gate_packing_pairs_partners_32_apart():
    wg = wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=128, kernel_size=3))
    pk = wg._packed(torch.device('cpu'))
    w = wg.WN[0].in_layers[1].weight.detach().permute(0, 2, 1).reshape(256, 384)
    pw = pk['flows'][0]['in_w'][1]
    for q in range(4):
        assert torch.equal(pw[64 * q:64 * q + 32], w[32 * q:32 * q + 32])
        assert torch.equal(pw[64 * q + 32:64 * q + 64], w[128 + 32 * q:128 + 32 * q + 32])


@contextlib.contextmanager
def _validate_only():
    native.set_validate_only(True)
    try:
        yield
    finally:
        native.set_validate_only(False)


def _err(fn, *args, match, **kw):
    with pytest.raises(native.NativeError, match=match):
        fn(*args, **kw)


def test_entry_points_reject_bad_arguments(native_lib):
    P, C, G = 80, 64, 8
    X, acts, skip, h = (torch.zeros(P, C) for _ in range(4))
    W = torch.zeros(2 * C, 3 * C)
    cnd = torch.zeros(P, 2 * C)
    rowb = torch.zeros(P, dtype=torch.int32)
    audio = torch.zeros(P, G)
    with _validate_only():
        native.wg_gated(X, W, torch.zeros(2 * C), 2, cnd, acts, 0)
        native.wg_res_skip(acts, torch.zeros(2 * C, C), torch.zeros(2 * C), h, skip, True, rowb, 1)
        native.wg_res_skip(acts, torch.zeros(C, C), torch.zeros(C), None, skip, False, rowb, 2)
        native.wg_tail(rowb, rowb, audio, G, z=torch.zeros(1, 4, P), start_w=torch.zeros(C, 2), start_b=torch.zeros(C), h=h)
        native.wg_denoise(torch.zeros(2, 5, 3), torch.zeros(5), 0.1)
        lib = native.load()
        nul = None
        _err(native._check, lib.t2amd_wg_layer_f32(nul, C, native.ptr(W), native.ptr(W), P, 2 * C, C, 3, 1, 0,
                                                    native.ptr(cnd), 2 * C, native.ptr(acts), C, nul, 0, 0, nul, 0, 0, nul,
                                                    0, nul), "x", match="null operand")
        _err(native.wg_gated, X, W, torch.zeros(2 * C), 2, cnd, acts, 3, match="precision")
        _err(native.wg_gated, torch.zeros(P, 48), torch.zeros(96, 144), torch.zeros(96), 2, torch.zeros(P, 96),
             torch.zeros(P, 48), 0, match="multiple of 32")
        _err(native.wg_gated, torch.zeros(P, 32), torch.zeros(64, 96), torch.zeros(64), 2, torch.zeros(P, 64),
             torch.zeros(P, 32), 0, match="multiple of 64")
        _err(native._check, lib.t2amd_wg_layer_f32(native.ptr(X), C, native.ptr(W), native.ptr(W), P, 2 * C, C, 1, 1, 2,
                                                    nul, 0, nul, 0, nul, 0, 0, native.ptr(skip), C, 0, native.ptr(rowb, torch.int32),
                                                    0, nul), "x", match="mode")
        _err(native._check, lib.t2amd_wg_layer_f32(native.ptr(X), C, native.ptr(W), native.ptr(W), P, 2 * C, C, 1, 1, 1,
                                                    nul, 0, nul, 0, nul, 0, C, native.ptr(skip), C, 0, native.ptr(rowb, torch.int32),
                                                    0, nul), "x", match="need h")
        _err(native.wg_tail, rowb, rowb, audio, G, start_w=torch.zeros(C, 2), start_b=torch.zeros(C), h=h,
             match="needs the noise")
        _err(native.wg_tail, rowb, rowb, audio, 7, z=torch.zeros(1, 4, P), match="n_group")
        _err(native.wg_tail, rowb, rowb, audio, G, z=torch.zeros(1, 4, P), out=torch.zeros(1, G * P), match="all n_group")
        _err(native.wg_tail, rowb, rowb, audio, G, skip=skip, end_w=torch.zeros(3, C), end_b=torch.zeros(3),
             winv=torch.zeros(3, 3), match="n_in")
        _err(native.wg_tail, rowb, rowb, torch.zeros(P, 4), G, z=torch.zeros(1, 4, P), match="audio rows")
        _err(native.wg_tail, rowb, rowb, audio, G, skip=skip, end_w=torch.zeros(4, 600), end_b=torch.zeros(4),
             winv=torch.zeros(4, 4), match="C must")
        _err(native.wg_denoise, torch.zeros(2, 5, 3), torch.zeros(4), 0.1, match="bins")
        _err(native._check, lib.t2amd_wg_denoise_f32(nul, native.ptr(skip), 1, 1, 1, 0.1, nul), "x", match="null operand")


# ---------------------------------------------------------------------------------------------------------------
# csrc/waveglow.hip on the host stand-in
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def waveglow_emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("waveglow_emu") / "libwaveglow_emu.so")
    src = [os.path.join(gu.ROOT, "tacotron2_amd", "csrc", "waveglow.hip"), os.path.join(EMU, "emu_runtime.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g0", "-w", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           "-I", EMU, "-x", "c++"] + src + ["-o", out])
    emu = ctypes.CDLL(out)
    assert emu.t2amd_emulated() == 1
    for name, at in native._argtypes().items():
        if hasattr(emu, name):
            fn = getattr(emu, name)
            fn.argtypes, fn.restype = at, ctypes.c_int
    emu.t2amd_last_error.restype = ctypes.c_char_p
    return emu


def _shifted(X, off):
    """rows m + off of the image X continues into (X is a view inside a larger buffer)."""
    return torch.as_strided(X, X.shape, X.stride(), X.storage_offset() + off * X.stride(0))


@contextlib.contextmanager
def _emulated(emu):
    names = ("gemm", "transpose", "wg_gated", "wg_res_skip")
    saved = (native._lib, native._validate_only) + tuple(getattr(native, n) for n in names)

    def gemm_standin(Cm, A, B, bias=None, convA=None, fast=0, **kw):
        A64 = A.double()
        if convA is not None:
            T, Cc, pad, sign = convA
            M = A.shape[0]
            t = torch.arange(M) % T
            cols = []
            for tap in range(B.shape[1] // Cc):
                sh = (tap - pad) * sign
                ok = (t + sh >= 0) & (t + sh < T)
                s = torch.zeros(M, Cc, dtype=torch.float64)
                s[ok] = A64[torch.arange(M)[ok] + sh]
                cols.append(s)
            A64 = torch.cat(cols, 1)
        r = A64 @ B.double().t()
        if bias is not None:
            r = r + bias.double()
        Cm.copy_(r)

    def transpose_standin(dst, src, batch=1, sstride=0, dstride=0):
        for b in range(batch):
            s = torch.as_strided(src, src.shape, src.stride(), src.storage_offset() + b * sstride)
            d = torch.as_strided(dst, dst.shape, dst.stride(), dst.storage_offset() + b * dstride)
            d.copy_(s.t())

    def gated_standin(X, W, bias, dil, cnd, acts, precision):
        C = acts.shape[1]
        A = torch.cat([_shifted(X, -dil), X, _shifted(X, dil)], 1).double()
        pre = (A @ W.double().t() + bias.double()).view(-1, C // 32, 2, 32)
        t = pre[:, :, 0].reshape(-1, C) + cnd[:, :C].double()
        s = pre[:, :, 1].reshape(-1, C) + cnd[:, C:].double()
        acts.copy_(torch.tanh(t) * torch.sigmoid(s))

    def res_skip_standin(acts, W, bias, h, skip, skip_store, rowb, precision):
        r = acts.double() @ W.double().t() + bias.double()
        nres = 0
        if h is not None:
            nres = h.shape[1]
            ok = rowb[:h.shape[0]] >= 0
            h[ok] = (h.double()[ok] + r[ok, :nres]).float()
        skip.copy_(r[:, nres:] if skip_store else skip.double() + r[:, nres:])

    native._lib, native._validate_only = emu, True           # CPU pointers allowed, kernels DO run (emulated)
    native.gemm, native.transpose, native.wg_gated, native.wg_res_skip = (gemm_standin, transpose_standin, gated_standin,
                                                                          res_skip_standin)
    try:
        yield
    finally:
        native._lib, native._validate_only = saved[:2]
        for n, f in zip(names, saved[2:]):
            setattr(native, n, f)


def test_emulated_flow_tail_ragged_matches_float64(waveglow_emu):
    rs = np.random.RandomState(0)
    wg = wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=3))
    lens = [1, 3, 2]
    N, G, C, H = 3, 8, 64, wg.halo()
    rowb, rowr, offs, P = wg.packed_plan(lens)
    assert P == H + sum(32 * n + H for n in lens) and offs[0] == H
    skip = torch.from_numpy(rs.randn(P, C).astype(np.float32))
    end_w = torch.from_numpy((0.05 * rs.randn(6, C)).astype(np.float32))
    end_b = torch.from_numpy((0.05 * rs.randn(6)).astype(np.float32))
    winv = torch.from_numpy(rs.randn(6, 6).astype(np.float32))
    audio0 = torch.from_numpy(rs.randn(P, G).astype(np.float32))
    z = torch.from_numpy(rs.randn(3, 2, 32 * N).astype(np.float32))
    start_w = torch.from_numpy(rs.randn(C, 4).astype(np.float32))
    start_b = torch.from_numpy(rs.randn(C).astype(np.float32))
    sentinel = 7.0
    audio = audio0.clone()
    h = torch.zeros(P, C)
    valid = (rowb >= 0).numpy()
    h[torch.from_numpy(~valid)] = 0.0
    with _emulated(waveglow_emu):
        native.wg_tail(rowb, rowr, audio, G, skip=skip, end_w=end_w, end_b=end_b, winv=winv, z=z, sigma=0.5,
                       start_w=start_w, start_b=start_b, h=h)
        out = torch.full((3, 256 * N), sentinel)
        audio2 = audio0.clone()
        audio2[:, 6:] = 0.0
        native.wg_tail(rowb, rowr, audio2, G, skip=skip, end_w=torch.cat([end_w, end_w[:2]]),
                       end_b=torch.cat([end_b, end_b[:2]]), winv=torch.eye(8), out=out)
    # float64 numpy restatement
    sk, a0 = skip.numpy().astype(np.float64), audio0.numpy().astype(np.float64)
    e = sk @ end_w.numpy().astype(np.float64).T + end_b.numpy()
    x = a0[:, :6].copy()
    x[:, 3:] = (x[:, 3:] - e[:, :3]) / np.exp(e[:, 3:])
    y = x @ winv.numpy().astype(np.float64).T
    zz = np.zeros((P, 2))
    for p in np.nonzero(valid)[0]:
        zz[p] = 0.5 * z.numpy()[rowb[p], :, rowr[p]]
    a = np.concatenate([zz, y], 1)
    hh = a[:, :4] @ start_w.numpy().astype(np.float64).T + start_b.numpy()
    got_a, got_h = audio.numpy(), h.numpy()
    assert np.abs(got_a[valid] - a[valid]).max() < 1e-5 * max(1.0, np.abs(a[valid]).max())
    assert np.abs(got_h[valid] - hh[valid]).max() < 1e-5 * max(1.0, np.abs(hh[valid]).max())
    assert not got_h[~valid].any(), "halo rows of h must stay zero"
    assert np.array_equal(got_a[~valid], a0[~valid]), "halo rows of audio must be untouched"
    # the waveform: sample 8 r + g of utterance b, untouched beyond 256 n_b
    o = out.numpy()
    e2 = np.concatenate([e, e[:, :2]], 1)
    x2 = a0.copy()
    x2[:, 6:] = 0.0
    x2[:, 4:] = (x2[:, 4:] - e2[:, :4]) / np.exp(e2[:, 4:])
    for b, n in enumerate(lens):
        rows = np.arange(offs[b], offs[b] + 32 * n)
        assert np.abs(o[b, :256 * n] - x2[rows].reshape(-1)).max() < 1e-5 * max(1.0, np.abs(x2).max())
        assert (o[b, 256 * n:] == sentinel).all()


@pytest.mark.parametrize("ragged", [False, True])
def test_emulated_infer_matches_restatement(waveglow_emu, ragged):
    ref = _small_ref(seed=5)
    wg = wgm.WaveGlow.from_module(ref)
    g = torch.Generator().manual_seed(6)
    B, N = 2, 3
    mel = torch.randn(B, 80, N, generator=g)
    lens = [3, 2] if ragged else None
    zs = [torch.randn(s, generator=g) for s in wg.noise_shapes(B, N)]
    with _emulated(waveglow_emu):
        out = wg.infer(mel, sigma=0.7, lengths=lens, z=zs)
    assert out.shape == (B, 256 * N) and out.dtype == torch.float32
    s_max, b_max = wr.coupling_stats(ref, mel.double(), 0.7, [t.double() for t in zs])
    print("couplings: max |s| %.3g, max |b| %.3g" % (s_max, b_max))
    assert s_max > 1e-2 and b_max > 1e-2
    for b in range(B):
        n = lens[b] if ragged else N
        want = ref.infer(mel[b:b + 1, :, :n].double(), 0.7, [t[b:b + 1, :, :32 * n].double() for t in zs])[0]
        got = out[b, :256 * n].double()
        rel = ((got - want).norm() / want.norm()).item()
        print("utterance %d: relative L2 %.3g" % (b, rel))
        assert rel < 1e-5
        assert not out[b, 256 * n:].any()
