"""The backward pass of the Vocos vocoder without a GPU: the differentiable restatement (tests/vocos_grad_ref.py) against
``VocosRef.forward`` and gradcheck, the models of the formulas of csrc/vocos_bwd.hip against float64 autograd of their forward
pieces, that very source run on the host stand-in against the models, the entries' argument checks in validate-only mode, the
kept-state accounting, and the clamp condition of every case the GPU tests run."""
import contextlib
import ctypes
import importlib.util
import math
import os

import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import vocos_grad_ref as gr
import vocos_ref as vr
from tacotron2_amd import native
from tacotron2_amd import vocos as vc

LENS = [3, 1, 140]
TINY = dict(n_mel_channels=3, dim=32, intermediate_dim=32, num_layers=1, n_fft=32, hop_length=8, padding='same')


def _module(name, seed=1):
    ref = vr.make_ref(name, seed)
    c = ref.config
    return ref, vc.load_vocos(ref.state_dict(), hop_length=c['hop_length'], padding=c['padding'])


def _close(a, b, tol=1e-11):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


# ---- the composition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ['small', 'center'])
def test_composition_is_the_restatement(name):
    ref = vr.make_ref(name, 3)
    mel = vr.make_mel(2, 9, 4, ref.config['n_mel_channels']).double()
    assert torch.equal(gr.audio(ref, mel), ref(mel))
    rag = gr.audio(ref, mel, [9, 1 if name == 'small' else 2])
    assert torch.equal(rag[0:1], ref(mel[0:1]))
    n1 = 1 if name == 'small' else 2
    alone = ref(mel[1:2, :, :n1])
    assert torch.equal(rag[1:2, :, :alone.shape[2]], alone) and not rag[1, :, alone.shape[2]:].any()


def test_gradcheck_on_a_tiny_geometry():
    for padding in vc.PADDINGS:
        ref = vr.make_ref(dict(TINY, padding=padding), 5)
        names = [n for n, _, _ in vr.shapes(ref.config)]
        mel = vr.make_mel(1, 4, 6, 3).double().requires_grad_(True)
        m = gr.log_magnitudes(ref, mel.detach())
        assert (m - math.log(vr.CLAMP)).abs().min() > 1e-3            # central differences must not cross the clamp

        def fn(mel, *ws):
            w = dict(zip(names, ws))
            w['head.istft.window'] = ref.w['head.istft.window']
            return gr.audio(vr.VocosRef(ref.config, w), mel)

        ws = [ref.w[n].clone().requires_grad_(True) for n in names]
        assert torch.autograd.gradcheck(fn, [mel] + ws, eps=1e-6, atol=1e-6, rtol=1e-5)


# ---- the formulas ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", vc.PADDINGS)
def test_overlap_add_model_is_the_autograd_gradient(padding):
    m = vc.Vocos(**dict(vr.CONFIGS['small'], padding=padding))
    L, hop = m.n_fft, m.hop
    win = torch.hann_window(L, periodic=True, dtype=torch.float64)
    for lens in ([2, 5] + ([1] if padding == 'same' else []), [7]):
        rowb0, rowr0, utt, offs, P = m.packed_plan(lens)
        T = m.samples(max(lens))
        frames = torch.randn(P, L, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
        r = gr.loss_weights((len(lens), 1, T), 2)
        loss = 0.0
        for b, (o, n) in enumerate(zip(offs, lens)):
            fr = frames[o:o + n].t()[None]
            y, env = vr.overlap_add(fr, hop)[0], vr.overlap_add((win * win)[None, :, None].expand(1, L, n), hop)[0]
            t = m.trim()
            a = y[t:y.numel() - t] / env[t:y.numel() - t]             # trimmed first, as vocos_ref.istft: env is 0 at the ends
            assert a.numel() == m.samples(n)
            loss = loss + (a * r[b, 0, :a.numel()]).sum()
        loss.backward()
        _close(gr.ola_bwd(r, win * win, lens, offs, P, hop, m.trim()), frames.grad)


def test_polar_model_is_the_autograd_gradient_with_clamped_bins():
    g = torch.Generator().manual_seed(3)
    Fb = 9
    Y = torch.cat([torch.randn(12, Fb, generator=g, dtype=torch.float64) * 3 + 3, torch.randn(12, Fb, generator=g,
                                                                                               dtype=torch.float64) * 4], 1)
    Y.requires_grad_(True)
    dS = torch.randn(12, 2 * Fb, generator=g, dtype=torch.float64)
    mag = torch.clamp(torch.exp(Y[:, :Fb]), max=vr.CLAMP)
    assert 0.1 < (mag == vr.CLAMP).double().mean() < 0.9
    S = torch.stack([mag * torch.cos(Y[:, Fb:]), mag * torch.sin(Y[:, Fb:])], 2).reshape(12, 2 * Fb)
    (S * dS).sum().backward()
    _close(gr.polar_bwd(Y.detach(), dS, Fb), Y.grad)
    assert not gr.polar_bwd(Y.detach(), dS, Fb)[:, :Fb][mag == vr.CLAMP].any()


def _block_images(D, I, seed, dtype=torch.float64):
    m = vc.Vocos(**vr.CONFIGS['small'])
    rowb0, rowr0, utt, offs, P = m.packed_plan(LENS)
    real = rowb0 >= 0
    g = torch.Generator().manual_seed(seed)

    def img(C, scale=1.0):
        return (scale * torch.randn(P, C, generator=g, dtype=torch.float64) * real[:, None]).to(dtype)

    return m, rowb0, rowr0, utt, offs, P, real, g, img


def test_layernorm_dwconv_gelu_gamma_models_are_the_autograd_gradients():
    D, I = 32, 64
    m, rowb0, rowr0, utt, offs, P, real, g, img = _block_images(D, I, 4)
    X = img(D, 2.0) + 0.5 * real[:, None]
    w = torch.randn(7, D, generator=g, dtype=torch.float64) / 7 ** 0.5
    cb, lw, lb, gamma = [torch.randn(D, generator=g, dtype=torch.float64) * 0.3 + o for o in (0.0, 1.0, 0.0, 0.0)]
    G, res = img(D), img(D)
    leaves = [t.requires_grad_(True) for t in (X, w, cb, lw, lb)]
    want_dx = torch.zeros_like(X)
    loss = 0.0
    for o, n in zip(offs, LENS):                                      # every utterance alone, with torch's own modules
        x = X[o:o + n].t()[None]
        y = F.conv1d(x, w.t()[:, None, :], cb, padding=3, groups=D)
        out = vr.layer_norm(y, lw, lb)[0].t()
        loss = loss + (out * G[o:o + n]).sum() + (X[o:o + n] * res[o:o + n]).sum()
    loss.backward()
    Xd, wd = X.detach(), w.detach()
    y = gr.dwconv(Xd, wd, cb.detach(), real)
    dz, dlw, dlb = gr.ln_bwd(y, lw.detach(), G, real)
    dx, dw, db = gr.dw_bwd(dz, Xd, wd, res, real)
    _close(dx, X.grad)
    _close(dw, w.grad)
    _close(db, cb.grad)
    _close(dlw, lw.grad)
    _close(dlb, lb.grad)
    # LayerNorm alone (backbone.norm, final_layer_norm)
    X2 = (img(D, 2.0) + 0.5 * real[:, None]).requires_grad_(True)
    lw2 = lw.detach().clone().requires_grad_(True)
    (F.layer_norm(X2[real], (D,), lw2, lb.detach(), vr.LN_EPS) * G[real]).sum().backward()
    dz2, dlw2, _ = gr.ln_bwd(X2.detach(), lw2.detach(), G, real)
    _close(dz2, X2.grad)
    _close(dlw2, lw2.grad)
    # GELU and gamma
    u, dh = img(I, 2.0).requires_grad_(True), img(I)
    (u * 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) * dh).sum().backward()
    _close(gr.gelu_bwd(u.detach(), dh), u.grad)
    y2, gm, dxx = img(D).requires_grad_(True), gamma.clone().requires_grad_(True), img(D)
    ((gm * y2) * dxx).sum().backward()
    dy2, dg = gr.gamma_bwd(dxx, y2.detach(), gm.detach())
    _close(dy2, y2.grad)
    _close(dg, gm.grad)


# ---- csrc/vocos_bwd.hip on the host stand-in ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bwd_emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_vocos_bwd_emu",
                                                  os.path.join(gu.ROOT, "tests", "hip_emu", "build_vocos_bwd_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    emu = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("vocos_bwd_emu"))))
    assert emu.t2amd_emulated() == 1
    for name, at in native._argtypes().items():
        if hasattr(emu, name):
            fn = getattr(emu, name)
            fn.argtypes, fn.restype = at, ctypes.c_int
    emu.t2amd_last_error.restype = ctypes.c_char_p
    return emu


@contextlib.contextmanager
def _emulated(emu):
    saved = (native._lib, native._validate_only)
    native._lib, native._validate_only = emu, True            # CPU pointers allowed, kernels DO run (emulated)
    try:
        yield
    finally:
        native._lib, native._validate_only = saved


def _sum_slots(partial, slots, n):
    return partial[:slots * n].view(slots, n).double().sum(0)


def _near(got, want, tol):
    """f32 kernels against the float64 models: sums of at most a few hundred terms of order 1."""
    assert got.shape == want.shape
    assert (got.double() - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("name", ['small', 'odd', 'center'])
def test_emulated_backward_kernels_equal_the_models(bwd_emu, name):
    lens = LENS if name != 'center' else [3, 2, 140]                  # 'center': one frame gives no sample
    ref, m = _module(name, seed=6)
    c = ref.config
    D, I, L, hop, Fb = c['dim'], c['intermediate_dim'], c['n_fft'], c['hop_length'], c['n_fft'] // 2 + 1
    rowb0, rowr0, utt, offs, P = m.packed_plan(lens)
    real = rowb0 >= 0
    g = torch.Generator().manual_seed(8)

    def img(C, scale=1.0):
        return scale * torch.randn(P, C, generator=g) * real[:, None]

    slots = -(-P // 16)
    T = m.samples(max(lens))
    d_audio = gr.loss_weights((len(lens), 1, T), 9).float()
    wsq = (ref.w['head.istft.window'] ** 2).float()
    d_frames = torch.full((P, L), 7.0)
    nh, ns = vc._pad_cols(2 * Fb), -(-2 * Fb // 32) * 32
    Y = torch.cat([torch.randn(P, Fb, generator=g) * 3 + 3, torch.randn(P, Fb, generator=g) * 8, torch.zeros(P, nh - 2 * Fb)], 1)
    dS, dY = img(ns), torch.full((P, nh), 7.0)
    u, dh = img(I, 2.0), img(I) + (~real)[:, None] * 7.0               # a stale halo must leave as zero
    dh0 = dh.clone()
    dxg, y2, gamma = img(D), img(D), torch.randn(D, generator=g) * 0.5
    y2_0 = y2.clone()
    X = img(D, 2.0) + 0.5 * real[:, None]
    w = torch.randn(7, D, generator=g) / 7 ** 0.5
    cb, lw = torch.randn(D, generator=g) * 0.1, torch.randn(D, generator=g) * 0.1 + 1.0
    G, res = img(D), img(D)
    dz, dz0, dx = torch.full((P, D), 7.0), torch.full((P, D), 7.0), torch.full((P, D), 7.0)
    p_g, p_ln, p_ln0, p_dw = [torch.full((slots * k * D,), 7.0) for k in (1, 2, 2, 8)]
    with _emulated(bwd_emu):
        assert native.vc_bwd_slot_rows() == 16 and native.vc_bwd_slots(P) == slots
        native.vc_ola_bwd(d_audio, wsq, utt, rowb0, rowr0, hop, m.trim(), d_frames)
        native.vc_polar_bwd(Y, Fb, vr.CLAMP, dS, rowb0, dY)
        native.vc_gelu_bwd(u, rowb0, dh)
        native.vc_gamma_bwd(dxg, gamma, rowb0, y2, p_g)
        native.vc_ln_bwd(X, w, cb, lw, vr.LN_EPS, rowb0, G, dz, p_ln)
        native.vc_ln_bwd(X, None, None, lw, vr.LN_EPS, rowb0, G, dz0, p_ln0)
        native.vc_dw_bwd(dz, X, w, rowb0, res, dx, p_dw)
    for out in (d_frames, dY, dh, y2, dz, dz0, dx):
        assert not out[~real].any(), "halo rows must be exactly zero"
    assert not dY[:, 2 * Fb:].any()
    dd = lambda t: t.double()
    _near(d_frames, gr.ola_bwd(dd(d_audio), dd(wsq), lens, offs, P, hop, m.trim()), 1e-6)
    mag = torch.clamp(torch.exp(dd(Y[:, :Fb])), max=vr.CLAMP)
    assert (mag[real] == vr.CLAMP).any() and (mag[real] < vr.CLAMP).any()
    _near(dY[:, :2 * Fb], gr.polar_bwd(dd(Y), dd(dS), Fb) * real[:, None], 4e-7 * vr.CLAMP * 8)
    _near(dh, gr.gelu_bwd(dd(u), dd(dh0)) * real[:, None], 1e-6)
    want_dy2, want_dg = gr.gamma_bwd(dd(dxg), dd(y2_0), dd(gamma))
    _near(y2, want_dy2, 1e-6)
    _near(_sum_slots(p_g, slots, D), want_dg, 1e-5)
    yd = gr.dwconv(dd(X), dd(w), dd(cb), real)
    wdz, wdlw, wdlb = gr.ln_bwd(yd, dd(lw), dd(G), real)
    _near(dz, wdz, 1e-5)
    _near(_sum_slots(p_ln, slots, 2 * D), torch.cat([wdlw, wdlb]), 1e-5)
    wdz0, wdlw0, wdlb0 = gr.ln_bwd(dd(X), dd(lw), dd(G), real)
    _near(dz0, wdz0 * real[:, None], 1e-5)
    _near(_sum_slots(p_ln0, slots, 2 * D), torch.cat([wdlw0, wdlb0]), 1e-5)
    wdx, wdw, wdb = gr.dw_bwd(dd(dz), dd(X), dd(w), dd(res), real)
    _near(dx, wdx, 1e-5)
    _near(_sum_slots(p_dw, slots, 8 * D), torch.cat([wdw.flatten(), wdb]), 1e-5)


# ---- validate-only: the entries' argument checks and the module's plumbing -------------------------------------------------
def _err(fn, *a, match):
    with pytest.raises(native.NativeError, match=match):
        fn(*a)


def test_backward_entries_reject_bad_arguments(native_lib):
    native.set_validate_only(True)
    try:
        z = torch.zeros
        P, D, I, L, Fb = 24, 64, 96, 64, 33
        rowb, rowr = torch.zeros(P, dtype=torch.int32), torch.zeros(P, dtype=torch.int32)
        utt = torch.tensor([[3, 18]], dtype=torch.int32)
        slots = native.vc_bwd_slots(P)
        X, G, dZ, dX, w, v = z(P, D), z(P, D), z(P, D), z(P, D), z(7, D), z(D)
        part = z(slots * 8 * D)
        bad_ld = z(P, D + 2)[:, :D]
        native.vc_ln_bwd(X, w, v, v, 1e-6, rowb, G, dZ, part)
        native.vc_ln_bwd(X, None, None, v, 1e-6, rowb, G, G, part)
        _err(native.vc_ln_bwd, X, w, v, v, 1e-6, rowb, G, X, part, match="must not be X")
        _err(native.vc_ln_bwd, X, w, v, v, 1e-6, rowb[:5], G, dZ, part, match="row map")
        _err(native.vc_ln_bwd, X, z(9, D), v, v, 1e-6, rowb, G, dZ, part, match="at most 7")
        _err(native.vc_ln_bwd, z(P, 48), None, None, z(48), 1e-6, rowb, z(P, 48), z(P, 48), part, match="multiple of 32")
        _err(native.vc_ln_bwd, X, w, v, v, 1e-6, rowb, bad_ld, dZ, part, match="multiple of 4")
        _err(native.vc_ln_bwd, X, w, v, v, 1e-6, rowb, G, dZ, None, match="null operand")
        _err(native.vc_ln_bwd, X, w, v, v, 1e-6, rowb, G, dZ, part[:slots * 2 * D - 1], match="partial is shorter")
        _err(native.vc_ln_bwd, X, w, v, v, 0.0, rowb, G, dZ, part, match="eps")
        native.vc_dw_bwd(dZ, X, w, rowb, None, dX, part)
        native.vc_dw_bwd(dZ, X, w, rowb, dX, dX, part)
        _err(native.vc_dw_bwd, dZ, X, w, rowb, None, dZ, part, match="must not be d_Z or X")
        _err(native.vc_dw_bwd, dZ, X, z(9, D), rowb, None, dX, z(slots * 10 * D), match="at most 7")
        _err(native.vc_dw_bwd, dZ, bad_ld, w, rowb, None, dX, part, match="multiple of 4")
        _err(native.vc_dw_bwd, z(P, 48), z(P, 48), z(7, 48), rowb, None, z(P, 48), part, match="multiple of 32")
        _err(native.vc_dw_bwd, dZ, X, w, rowb, None, dX, None, match="null operand")
        _err(native.vc_dw_bwd, dZ, X, w, rowb, None, dX, part[:slots * 8 * D - 1], match="partial is shorter")
        native.vc_gamma_bwd(dX, v, rowb, dZ, part)
        _err(native.vc_gamma_bwd, dX, v, rowb, dX, part, match="two buffers")
        _err(native.vc_gamma_bwd, dX, v, rowb, bad_ld, part, match="multiple of 4")
        _err(native.vc_gamma_bwd, z(P, 48), z(48), rowb, z(P, 48), part, match="multiple of 32")
        _err(native.vc_gamma_bwd, dX, v, rowb, dZ, None, match="null operand")
        _err(native.vc_gamma_bwd, dX, z(D + 1), rowb, dZ, part, match="shape mismatch")
        U, dH = z(P, I), z(P, I)
        native.vc_gelu_bwd(U, rowb, dH)
        _err(native.vc_gelu_bwd, U, rowb, U, match="two buffers")
        _err(native.vc_gelu_bwd, z(P, 48), rowb, z(P, 48), match="multiple of 32")
        _err(native.vc_gelu_bwd, z(P, I + 2)[:, :I], rowb, dH, match="multiple of 4")
        _err(native.vc_gelu_bwd, U, rowb[:5], dH, match="row map")
        _err(native.vc_gelu_bwd, U, rowb, z(P, D), match="shape mismatch")
        Y, dS, dY = z(P, 96), z(P, 96), z(P, 96)
        native.vc_polar_bwd(Y, Fb, 100.0, dS, rowb, dY)
        _err(native.vc_polar_bwd, Y, Fb, 100.0, dS, rowb, Y, match="one of the inputs")
        _err(native.vc_polar_bwd, Y, Fb, 0.0, dS, rowb, dY, match="positive clamp")
        _err(native.vc_polar_bwd, Y, 49, 100.0, dS, rowb, dY, match="shape mismatch")
        _err(native.vc_polar_bwd, Y, Fb, 100.0, dS, rowb[:5], dY, match="row map")
        d_audio, wsq, fr = z(1, 1, 16 * 18), z(L), z(P, L)
        native.vc_ola_bwd(d_audio, wsq, utt, rowb, rowr, 16, 24, fr)
        _err(native.vc_ola_bwd, d_audio, wsq, utt, rowb, rowr, 24, 20, fr, match="multiple of 4")
        _err(native.vc_ola_bwd, d_audio, wsq, utt, rowb, rowr, 16, 8, fr, match="trim")
        _err(native.vc_ola_bwd, d_audio, wsq, utt, rowb, rowr, 16, 24, z(P, L + 2)[:, :L], match="16-byte aligned rows")
        _err(native.vc_ola_bwd, d_audio, z(L - 1), utt, rowb, rowr, 16, 24, fr, match="shape mismatch")
        _err(native.vc_ola_bwd, d_audio, wsq, utt, rowb[:5], rowr[:5], 16, 24, fr, match="row map")
    finally:
        native.set_validate_only(False)


@pytest.mark.parametrize("name", ['small', 'odd', 'center'])
def test_generate_and_backward_pass_every_entrys_checks_validate_only(native_lib, name, monkeypatch):
    _, m = _module(name)
    calls = []
    for fn in ('vc_ola_bwd', 'vc_polar_bwd', 'vc_gelu_bwd', 'vc_gamma_bwd', 'vc_ln_bwd', 'vc_dw_bwd'):
        real = getattr(native, fn)
        monkeypatch.setattr(native, fn, (lambda real, fn: lambda *a, **k: (calls.append(fn), real(*a, **k))[1])(real, fn))
    native.set_validate_only(True)
    try:
        nm, L = m.n_mel_channels, m.num_layers
        for prec in ('fp32', 'bf16x3', 'bf16'):
            m.precision = prec
            del calls[:]
            mel = vr.make_mel(3, 40, 1, nm).requires_grad_(True)
            out = m.generate(mel, lengths=[2, 7, 40])
            assert out.shape == (3, 1, m.samples(40)) and out.dtype == torch.float32 and out.grad_fn is not None
            out.sum().backward()
            assert calls == ['vc_ola_bwd', 'vc_polar_bwd', 'vc_ln_bwd'] + ['vc_gamma_bwd', 'vc_gelu_bwd', 'vc_ln_bwd',
                                                                            'vc_dw_bwd'] * L + ['vc_ln_bwd']
            assert mel.grad.shape == mel.shape and mel.grad.dtype == torch.float32
            for n, p in m.named_parameters():
                assert p.grad is not None and p.grad.shape == p.shape, n
            assert m.head.istft.window.grad is None and not m.head.istft.window.requires_grad
            m.zero_grad()
        with torch.no_grad():
            assert m.generate(vr.make_mel(1, 5, 1, nm)).grad_fn is None
        for p in m.parameters():
            p.requires_grad_(False)
        assert m.generate(vr.make_mel(1, 5, 1, nm)).grad_fn is None
        with pytest.raises(ValueError, match="training keeps float32"):
            m.half().generate(vr.make_mel(1, 5, 1, nm))
        m.float()
        with pytest.raises(ValueError, match="lengths"):
            m.generate(vr.make_mel(1, 5, 1, nm).requires_grad_(True), lengths=[6])
    finally:
        native.set_validate_only(False)


def test_saved_state_bytes_layout_and_refusal():
    m = vc.Vocos(**vr.CONFIGS['V'])
    per_row = 96 + 19 * 512 + 8 * 1536 + 1152                        # ce(80) + (2 L + 3) D + L I + the head's padded columns
    assert m.saved_state_bytes(1) == 4 * per_row == 4 * sum(m.saved_row_widths())
    assert m.saved_state_bytes(876) == 876 * 4 * per_row
    s = vc.Vocos(**vr.CONFIGS['small'])
    assert s.saved_state_bytes(10) == 40 * (32 + 7 * 64 + 2 * 192 + 96)
    total, lay = s._grad_layout(2, 9)
    assert set(lay) == {n for n, _, _ in vr.shapes(s.config())} | {'mel'} and 'head.istft.window' not in lay
    assert all(o % 4 == 0 for o, _ in lay.values()) and lay['mel'][1] == (2, 20, 9)
    ends = sorted((o, o + int(torch.Size(sh).numel())) for o, sh in lay.values())
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] <= total
    for n in ('backbone.norm', 'backbone.final_layer_norm', 'backbone.convnext.1.norm'):
        assert lay[n + '.bias'][0] == lay[n + '.weight'][0] + 64       # one ordered pass sums both
    m._check_state(10 ** 9, 10 ** 8, 2 * 10 ** 9, 100)
    with pytest.raises(native.NativeError, match=r"Vocos.generate: the state kept for the backward pass needs 1.00 GB \(100 "
                                                 r"packed rows x 23264 floats\) and 1.05 GB are free; use a smaller batch"):
        m._check_state(10 ** 9, 10 ** 8, 1.05 * 10 ** 9, 100)


# ---- the clamp condition of the GPU cases ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lens,seed", gr.GPU_CASES)
def test_no_reference_log_magnitude_sits_at_the_clamp(name, lens, seed):
    """No float64 log-magnitude of a GPU case lies within the case's margin of log(100) (tests/vocos_grad_ref.py says why
    and which margin), and both sides of the clamp occur."""
    ref = vr.make_ref(name, gr.WEIGHT_SEED)
    mel = vr.make_mel(len(lens), max(lens), seed, ref.config['n_mel_channels']).double()
    m = gr.log_magnitudes(ref, mel, lens if len(set(lens)) > 1 else None)
    gap = (m - math.log(vr.CLAMP)).abs().min().item()
    assert gr.clamp_margin(name) >= gr.CLAMP_MARGIN and gap > gr.clamp_margin(name), (name, lens, seed, gap)
    assert (m > math.log(vr.CLAMP)).any() and (m < math.log(vr.CLAMP)).any()


def test_one_bin_on_the_other_side_of_the_clamp_moves_the_gradients_by_a_tenth():
    """Why the margin: with mel seed 2 the ragged case has bins 2.3e-3 and 2.7e-3 above log(100) in float64; the bf16 mode on
    the MI355X put both below it and its gradients were off by 0.13 to 0.16 in relative L2 (mels 0.1601), ten times the
    other cases.  In float64, inverting the clamp side of exactly these two bins moves the gradients by the same amounts."""
    name, lens, seed, flips = 'small', [3, 1, 140], 2, [(2, 28, 44), (2, 28, 64)]
    ref = vr.make_ref(name, gr.WEIGHT_SEED)
    mel = vr.make_mel(3, 140, seed, 20).double()
    m = ref.head(ref.backbone(mel[2:3]))[0][0] - math.log(vr.CLAMP)
    assert all(0 < m[k, j].item() < 3e-3 for _, k, j in flips)
    r = gr.loss_weights((3, 1, 16 * 140), seed + 100)
    g, gf = gr.grads(ref, mel, r, lens), gr.grads(ref, mel, r, lens, flips)
    rel = {k: ((gf[k] - g[k]).norm() / g[k].norm()).item() for k in g}
    assert abs(rel['mel'] - 0.1601) < 0.005, rel['mel']
    assert abs(rel['backbone.convnext.0.norm.weight'] - 0.152) < 0.01 and abs(rel['head.out.bias'] - 0.1332) < 0.01, rel
