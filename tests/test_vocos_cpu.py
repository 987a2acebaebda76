"""The Vocos vocoder without a GPU: geometry from tensor shapes and loading, every refusal, the argument checks of the new
entry points (validate-only), a numpy model of which rows every launch reads, the float64 restatement against torch's own
istft / Conv1d / LayerNorm / GELU modules and its weight scales, csrc/vocos_rows.hip run on the host stand-in of tests/hip_emu
against float64, and the command line's argument handling."""
import contextlib
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
from torch import nn

import golden_util as gu
import vocos_ref as vr
from tacotron2_amd import native
from tacotron2_amd import vocos as vc

NAMES = ('small', 'odd', 'center', 'V')


def _load(name, seed=1):
    ref = vr.make_ref(name, seed)
    c = vr.CONFIGS[name]
    return ref, vc.load_vocos(ref.state_dict(), hop_length=c['hop_length'], padding=c['padding'])


# ---------------------------------------------------------------------------------------------------------------
# geometry and loading
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_geometry_from_shapes(name):
    ref = vr.make_ref(name, seed=1)
    c = vr.CONFIGS[name]
    sd = ref.state_dict()
    assert vc.config_from_state_dict(sd, padding=c['padding']) == c                  # hop defaults to n_fft / 4
    assert vc.config_from_state_dict(sd, hop_length=c['n_fft'] // 2)['hop_length'] == c['n_fft'] // 2
    m = vc.load_vocos(sd, precision='bf16x3', padding=c['padding'])
    assert m.config() == c and m.precision == 'bf16x3' and m.hop_length == c['hop_length']
    assert set(m.state_dict()) == set(sd)
    for k, v in m.state_dict().items():
        assert v.dtype == torch.float32 and torch.equal(v.double(), sd[k]), k


def test_sources_feature_extractor_adanorm_and_strict_loading(tmp_path):
    ref = vr.make_ref('small', seed=2)
    sd = ref.state_dict()
    m = vc.load_vocos(sd)
    assert vc.load_vocos(m) is m and m.precision == 'fp32'
    assert vc.load_vocos(m, precision='bf16x3', hop_length=16, padding='same') is m and m.precision == 'bf16x3'
    m.precision = 'fp32'
    for kw in (dict(hop_length=32), dict(padding='center')):
        with pytest.raises(ValueError, match="the module has hop 16"):
            vc.load_vocos(m, **kw)
    published = dict(sd)
    published['feature_extractor.mel_spec.spectrogram.window'] = torch.zeros(64)
    published['feature_extractor.mel_spec.mel_scale.fb'] = torch.zeros(33, 20)
    p = str(tmp_path / "v.pt")
    torch.save({'state_dict': published}, p)
    for src in (published, {'state_dict': published}, p):
        got = vc.load_vocos(src)
        assert not any(k.startswith('feature_extractor') for k in got.state_dict())
        for k, v in got.state_dict().items():
            assert torch.equal(v, m.state_dict()[k]), k
    foreign = nn.Module()                    # any module with the published submodule names
    foreign.backbone, foreign.head = m.backbone, m.head
    h = vc.load_vocos(foreign)
    assert h is not m and h.config() == m.config()
    with pytest.raises(TypeError):
        vc.load_vocos(3)
    ada = dict(sd)
    ada['backbone.norm.scale.weight'] = torch.zeros(4, 64)
    with pytest.raises(ValueError, match="adanorm"):
        vc.load_vocos(ada)
    with pytest.raises(ValueError, match="adanorm"):
        vc.load_vocos({'backbone.convnext.0.adanorm.scale.weight': torch.zeros(4, 64)})
    missing = {k: v for k, v in sd.items() if k != 'backbone.convnext.1.gamma'}
    with pytest.raises(RuntimeError, match="gamma"):
        vc.load_vocos(missing)
    extra = dict(sd, **{'head.extra': torch.zeros(1)})
    with pytest.raises(RuntimeError, match="head.extra"):
        vc.load_vocos(extra)
    with pytest.raises(ValueError, match="not a Vocos state dict"):
        vc.load_vocos({'conv_pre.weight': torch.zeros(4, 4, 7)})
    with pytest.raises(ValueError, match="does not match"):
        vc.Vocos(**dict(vr.CONFIGS['small'], dim=96)).load_state_dict(sd)
    with pytest.raises(ValueError, match="window"):
        vc.load_vocos(dict(sd, **{'head.istft.window': torch.zeros(32)}))


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change,msg", [
    (dict(dim=80), "dim 80"), (dict(dim=544), "dim 544"), (dict(intermediate_dim=100), "intermediate_dim 100"),
    (dict(intermediate_dim=2080), "intermediate_dim 2080"), (dict(n_fft=96, hop_length=3), "is odd"),
    (dict(n_fft=64, hop_length=24), "does not divide"), (dict(n_fft=64, hop_length=64), "must overlap"),
    (dict(n_fft=64, hop_length=8), "must overlap"), (dict(n_fft=72, hop_length=18), "n_fft 72"),
    (dict(padding='valid'), "padding"), (dict(precision='fp16'), "precision"), (dict(num_layers=0), "num_layers"),
    (dict(n_mel_channels=513), "n_mel_channels")])
def test_geometry_the_kernels_do_not_cover_is_refused(change, msg):
    with pytest.raises(ValueError, match=msg):
        vc.Vocos(**dict(vr.CONFIGS['small'], **change))


def test_bad_calls_are_refused(native_lib):
    _, m = _load('small')
    mel = vr.make_mel(2, 9, 1, 20)
    with pytest.raises(native.NativeError, match="no CPU path"):
        m.infer(mel)
    native.set_validate_only(True)
    try:
        assert m.infer(mel).shape == (2, 1, 16 * 9)
        for bad in (mel[0], vr.make_mel(2, 9, 1, 21), "mel"):
            with pytest.raises(ValueError, match="expected"):
                m.infer(bad)
        for bad in (mel.double(), mel.long()):
            with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
                m.infer(bad)
        for lens in ([9], [9, 10], [0, 9], [9, 9, 9]):
            with pytest.raises(ValueError, match="lengths"):
                m.infer(mel, lengths=lens)
        _, c = _load('center')
        assert c.infer(mel).shape == (2, 1, 16 * 8)
        with pytest.raises(ValueError, match="at least one sample"):
            c.infer(mel[:, :, :1])
    finally:
        native.set_validate_only(False)
    with pytest.raises(ValueError, match="precision"):
        m.precision = 'tf32'


# ---------------------------------------------------------------------------------------------------------------
# validate-only: host plumbing and the entries' argument checks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_infer_passes_every_entrys_checks_validate_only(native_lib, name, monkeypatch):
    _, m = _load(name)
    calls = []
    for fn in ('hg_pack_mel', 'hg_conv', 'vc_dwln', 'vc_linear', 'vc_polar', 'vc_ola'):
        real = getattr(native, fn)
        monkeypatch.setattr(native, fn, (lambda real, fn: lambda *a, **k: (calls.append(fn), real(*a, **k))[1])(real, fn))
    native.set_validate_only(True)
    try:
        nm = m.n_mel_channels
        for prec in ('fp32', 'bf16x3', 'bf16'):
            m.precision = prec
            del calls[:]
            out = m.infer(vr.make_mel(3, 40, 1, nm), lengths=[1, 7, 40])
            assert out.shape == (3, 1, m.samples(40)) and out.dtype == torch.float32
            L = m.num_layers
            assert calls == ['hg_pack_mel', 'hg_conv', 'vc_dwln'] + ['vc_dwln', 'vc_linear', 'vc_linear'] * L + \
                ['vc_dwln', 'vc_linear', 'vc_polar', 'vc_linear', 'vc_ola']
        assert m.half().infer(vr.make_mel(1, 5, 1, nm).half()).dtype == torch.float16 and m.precision == 'bf16'
        assert m.float().precision == 'fp32'
    finally:
        native.set_validate_only(False)


def _err(fn, *a, match):
    with pytest.raises(native.NativeError, match=match):
        fn(*a)


def test_entries_reject_bad_arguments(native_lib):
    native.set_validate_only(True)
    try:
        z = torch.zeros
        P, D, I = 24, 64, 96
        rowb = torch.zeros(P, dtype=torch.int32)
        X, out, w, v = z(P, D), z(P, D), z(7, D), z(D)
        native.vc_dwln(X, w, v, v, v, 1e-6, rowb, out)
        native.vc_dwln(X, None, None, v, v, 1e-6, rowb, out)
        _err(native.vc_dwln, X, w, v, v, v, 1e-6, rowb, X, match="must not be X")
        _err(native.vc_dwln, X, w, v, v, v, 1e-6, rowb[:5], out, match="row map")
        _err(native.vc_dwln, X, z(6, D), v, v, v, 1e-6, rowb, out, match="taps must be 0")
        _err(native.vc_dwln, z(P, 48), z(7, 48), z(48), z(48), z(48), 1e-6, rowb, z(P, 48), match="multiple of 32")
        _err(native.vc_dwln, z(P, 544), None, None, z(544), z(544), 1e-6, rowb, z(P, 544), match="at most 512")
        _err(native.vc_dwln, X, w, v, v, v, 0.0, rowb, out, match="eps")
        _err(native.vc_dwln, X, w, v, v, z(D + 1)[1:], 1e-6, rowb, out, match="16-byte aligned")
        _err(native.vc_dwln, X, w, v, v, z(D + 1), 1e-6, rowb, out, match="shape mismatch")
        _err(native.vc_dwln, z(P + 1, D)[:P].t().contiguous().t(), w, v, v, v, 1e-6, rowb, out, match="contiguous rows")
        lib = native.load()
        p, i32 = native.ptr, torch.int32
        _err(native._check, lib.t2amd_vc_dwln_f32(p(X), P * D - 1, D, P, D, p(w), 7 * D, p(v), 7, p(v), p(v), 1e-6, p(rowb, i32),
                                                   P, p(out), D, P * D, None), "x", match="X is shorter")
        _err(native._check, lib.t2amd_vc_dwln_f32(p(X), P * D, D, P, D, p(w), 7 * D, p(v), 7, p(v), p(v), 1e-6, p(rowb, i32),
                                                   P, p(out), D, P * D - 1, None), "x", match="out is shorter")
        _err(native._check, lib.t2amd_vc_dwln_f32(p(X), P * D, D, P, D, p(w), 7 * D - 1, p(v), 7, p(v), p(v), 1e-6,
                                                   p(rowb, i32), P, p(out), D, P * D, None), "x", match="w is shorter")
        _err(native._check, lib.t2amd_vc_dwln_f32(None, P * D, D, P, D, p(w), 7 * D, p(v), 7, p(v), p(v), 1e-6, p(rowb, i32),
                                                   P, p(out), D, P * D, None), "x", match="null operand")

        W, h, bi = z(I, D), z(P, I), z(I)
        for prec in (0, 1, 2):
            native.vc_linear(X, W, bi, 'gelu', None, None, h, rowb, prec)
            native.vc_linear(h, z(D, I), v, 'residual', v, out, out, rowb, prec)
        _err(native.vc_linear, X, W, bi, 'gelu', None, None, h, rowb, 3, match="precision")
        _err(native.vc_linear, X, W, bi, 'tanh', None, None, h, rowb, 0, match="epi")
        _err(native.vc_linear, X, W, bi, 'residual', None, None, h, rowb, 0, match="needs bias, gamma and res")
        _err(native.vc_linear, X, z(I, 32), bi, None, None, None, h, rowb, 0, match="shape mismatch")
        _err(native.vc_linear, X, z(D, D), v, None, None, None, X, rowb, 0, match="must not be X")
        _err(native.vc_linear, z(P, 48), z(I, 48), bi, None, None, None, h, rowb, 0, match="K must be a multiple of 32")
        _err(native.vc_linear, X, z(48, D), z(48), None, None, None, z(P, 48), rowb, 0, match="N must be a multiple of 32")
        _err(native.vc_linear, X, W, bi, None, None, None, h, rowb[:3], 0, match="row map")
        _err(native.vc_linear, X, W, bi, 'residual', bi, z(P, D), h, rowb, 0, match="res .* beside out")
        _err(native._check, lib.t2amd_vc_linear_f32(p(X), P * D, D, P, D, p(W), I * D - 1, p(bi), I, 0, None, None, 0, 0, p(h), I,
                                                     P * I, p(rowb, i32), P, 0, None), "x", match="W is shorter")
        _err(native._check, lib.t2amd_vc_linear_f32(p(X), P * D, D, P, D, p(W), I * D, p(bi), I, 0, None, None, 0, 0, p(h), I,
                                                     P * I - 1, p(rowb, i32), P, 0, None), "x", match="out is shorter")
        _err(native._check, lib.t2amd_vc_linear_f32(p(z(P * D + 4)[1:]), P * D, D, P, D, p(W), I * D, p(bi), I, 0, None, None,
                                                     0, 0, p(h), I, P * I, p(rowb, i32), P, 0, None), "x", match="16-byte aligned")

        F_, Y, S = 33, z(P, 96), z(P, 96)
        native.vc_polar(Y, F_, 100.0, rowb, S)
        _err(native.vc_polar, Y, 49, 100.0, rowb, S, match="shape mismatch")
        _err(native.vc_polar, Y, F_, 0.0, rowb, S, match="positive clamp")
        _err(native.vc_polar, Y, F_, 100.0, rowb[:3], S, match="row map")
        _err(native.vc_polar, Y, F_, 100.0, rowb, Y, match="same buffer")
        _err(native._check, lib.t2amd_vc_polar_f32(p(Y), P * 96, 96, P, F_, 100.0, p(rowb, i32), P, p(S), 67, P * 96, None), "x",
             match="even stride")
        _err(native._check, lib.t2amd_vc_polar_f32(p(Y), P * 96, 96, P, F_, 100.0, p(rowb, i32), P, p(S), 96, P * 96 - 1, None),
             "x", match="S is shorter")

        fr, wsq, utt, wave = z(P, 64), z(64), torch.tensor([[3, 5], [11, 9]], dtype=i32), z(2, 1, 16 * 9)
        native.vc_ola(fr, wsq, utt, 16, 24, wave)
        native.vc_ola(fr, wsq, utt, 16, 32, wave)
        _err(native.vc_ola, fr, wsq, utt, 24, 20, wave, match="hop must divide")
        _err(native.vc_ola, fr, wsq, utt, 16, 23, wave, match="trim")
        _err(native.vc_ola, fr, wsq, utt, 16, 33, wave, match="trim")
        _err(native.vc_ola, fr, wsq, utt[:1], 16, 24, wave, match="shape mismatch")
        _err(native.vc_ola, fr, wsq[:63], utt, 16, 24, wave, match="shape mismatch")
        _err(native._check, lib.t2amd_vc_ola_f32(p(fr), P * 64 - 1, 64, P, p(wsq), p(utt, i32), 2, 64, 16, 24, p(wave), 144, 288,
                                                  None), "x", match="frames is shorter")
        _err(native._check, lib.t2amd_vc_ola_f32(p(fr), P * 64, 64, P, p(wsq), p(utt, i32), 2, 64, 16, 24, p(wave), 144, 287,
                                                  None), "x", match="out is shorter")
        _err(native._check, lib.t2amd_vc_ola_f32(p(fr), P * 64, 64, P, p(wsq), None, 2, 64, 16, 24, p(wave), 144, 288, None),
             "x", match="null operand")
    finally:
        native.set_validate_only(False)


# ---------------------------------------------------------------------------------------------------------------
# the row plan: which rows does every launch read
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_no_window_and_no_overlap_add_span_reaches_anothers_rows(name):
    m = vc.Vocos(**vr.CONFIGS[name])
    lens = [7, 1, 3, 5]
    rowb0, rowr0, utt, offs, P = m.packed_plan(lens)
    rowb0, rowr0 = rowb0.numpy(), rowr0.numpy()
    H = vc.HALO
    assert H == 3 and P == H + sum(n + H for n in lens) and utt.tolist() == [[o, n] for o, n in zip(offs, lens)]
    for b, (o, n) in enumerate(zip(offs, lens)):
        assert (rowb0[o:o + n] == b).all() and (rowr0[o:o + n] == np.arange(n)).all() and (rowb0[o - H:o] == -1).all()
    assert (rowb0[-H:] == -1).all() and (rowb0 >= 0).sum() == sum(lens)
    windows = m.row_windows()
    assert len(windows) == m.num_layers + 2 and max(max(-lo, hi) for lo, hi in windows) == H

    def reaches(rowb):
        real = np.nonzero(rowb >= 0)[0]
        hit = False
        for lo, hi in windows:
            for off in range(lo, hi + 1):
                src = real + off
                if src.min() < 0 or src.max() >= rowb.size:
                    return True
                hit |= bool(((rowb[src] != rowb[real]) & (rowb[src] != -1)).any())
        # the samples of a frame: packed row p starts at sample p hop of the packed sample space and is n_fft samples long
        hop, L = m.hop, m.n_fft
        owner = np.repeat(rowb, hop)
        for p in real:
            span = owner[p * hop:p * hop + L]
            hit |= span.size < L or bool(((span != rowb[p]) & (span != -1)).any())
        return hit

    assert not reaches(rowb0)
    short = np.concatenate([np.full(H - 1, -1)] + [np.r_[np.full(n, b), np.full(H - 1, -1)] for b, n in enumerate(lens)])
    assert reaches(short)                   # with H = 2 both a 7-tap window and a last frame's tail reach the neighbour


# ---------------------------------------------------------------------------------------------------------------
# the restatement against torch's own modules, and the scales of its weights
# ---------------------------------------------------------------------------------------------------------------
def test_restated_istft_equals_torch_istft_and_same_is_center_shifted():
    g = torch.Generator().manual_seed(3)
    for L, hop, N in ((64, 16, 9), (128, 32, 5), (1024, 256, 6)):
        S = torch.complex(torch.randn(2, L // 2 + 1, N, generator=g, dtype=torch.float64),
                          torch.randn(2, L // 2 + 1, N, generator=g, dtype=torch.float64))
        win = torch.hann_window(L, periodic=True, dtype=torch.float64)
        center = vr.istft(S, win, hop, 'center')
        same = vr.istft(S, win, hop, 'same')
        assert center.shape == (2, hop * (N - 1)) and same.shape == (2, hop * N)
        S0 = S.clone()                                       # torch.istft insists on real DC and Nyquist bins; irfft ignores them
        S0[:, 0].imag.zero_()
        S0[:, -1].imag.zero_()
        want = torch.istft(S0, L, hop, L, win, center=True)
        assert (center - want).abs().max() < 1e-12 * max(1.0, want.abs().max().item())
        # 'same' keeps n_fft / 2 - (n_fft - hop) / 2 = hop / 2 more samples at each end: where both are defined they agree
        shift = L // 2 - (L - hop) // 2
        assert shift == hop // 2 and torch.equal(same[:, shift:shift + center.shape[1]], center)
        full = vr.overlap_add(torch.fft.irfft(S, L, dim=1) * win[None, :, None], hop)
        env = vr.overlap_add((win * win)[None, :, None].expand(1, L, N), hop)
        t0, t1 = (L - hop) // 2, L // 2
        assert torch.equal(same, (full / env)[:, t0:full.shape[1] - t0]) and torch.equal(center, (full / env)[:, t1:full.shape[1] - t1])


def test_restated_block_equals_torch_modules():
    for name in ('small', 'odd'):
        ref = vr.make_ref(name, seed=4)
        c = ref.config
        D, I = c['dim'], c['intermediate_dim']
        dw, ln = nn.Conv1d(D, D, 7, padding=3, groups=D).double(), nn.LayerNorm(D, eps=1e-6).double()
        p1, p2, act = nn.Linear(D, I).double(), nn.Linear(I, D).double(), nn.GELU()
        pre = 'backbone.convnext.1.'
        with torch.no_grad():
            for mod, key in ((dw, 'dwconv'), (ln, 'norm'), (p1, 'pwconv1'), (p2, 'pwconv2')):
                mod.weight.copy_(ref.w[pre + key + '.weight'])
                mod.bias.copy_(ref.w[pre + key + '.bias'])
            x = torch.randn(2, D, 11, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
            y = p2(act(p1(ln(dw(x).transpose(1, 2)))))
            want = x + (ref.w[pre + 'gamma'] * y).transpose(1, 2)
            got = vr.convnext_block(x, ref.w, pre)
        assert (got - want).abs().max() < 1e-12


@pytest.mark.parametrize("name,B,N", [('small', 2, 40), ('odd', 2, 40), ('center', 2, 40), ('V', 1, 64)])
def test_reference_weights_exercise_clamp_phase_wrap_and_level(name, B, N):
    ref = vr.make_ref(name, 0)
    mel = vr.make_mel(B, N, 1, ref.config['n_mel_channels']).double()
    with torch.no_grad():
        m, p = ref.head(ref.backbone(mel))
    out = ref(mel)
    clamped = (m > math.log(100.0)).double().mean().item()
    assert out.shape == (B, 1, ref.config['hop_length'] * (N if ref.config['padding'] == 'same' else N - 1))
    assert out.pow(2).mean().sqrt().item() > 0.05
    assert 0.001 < clamped < 0.05, clamped
    assert p.abs().max().item() > math.pi and (p.abs() > math.pi).double().mean().item() > 0.05
    for k, v in ref.state_dict().items():
        assert torch.equal(v, v.float().double()), k                     # a float32 module holds exactly these weights


def test_inverse_basis_is_the_windowed_irfft():
    for L in (64, 128, 1024):
        win = torch.hann_window(L, periodic=True)
        basis = vc.inverse_basis(win).double()
        F_ = L // 2 + 1
        assert basis.shape == (L, -(-2 * F_ // 32) * 32) and not basis[:, 2 * F_:].any()
        g = torch.Generator().manual_seed(L)
        S = torch.complex(torch.randn(3, F_, generator=g, dtype=torch.float64), torch.randn(3, F_, generator=g, dtype=torch.float64))
        rows = torch.zeros(3, basis.shape[1], dtype=torch.float64)
        rows[:, 0:2 * F_:2], rows[:, 1:2 * F_:2] = S.real, S.imag
        want = torch.fft.irfft(S, L, dim=1) * win.double()
        assert (rows @ basis.t() - want).abs().max() < 1e-7 * want.abs().max()      # the basis is stored in float32


# ---------------------------------------------------------------------------------------------------------------
# csrc/vocos_rows.hip on the host stand-in
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vocos_emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_vocos_emu", os.path.join(gu.ROOT, "tests", "hip_emu", "build_vocos_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    emu = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("vocos_emu"))))
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


def test_emulated_row_kernels_match_float64(vocos_emu):
    lens = [1, 7, 5]
    for name in ('small', 'odd', 'center'):
        ref, m = _load(name, seed=6)
        c = ref.config
        D, L, hop, F_ = c['dim'], c['n_fft'], c['hop_length'], c['n_fft'] // 2 + 1
        rowb0, rowr0, utt, offs, P = m.packed_plan(lens)
        real = rowb0 >= 0
        g = torch.Generator().manual_seed(7)
        X = torch.randn(P, D, generator=g) * 2.0 + 0.5
        X[~real] = 0.0
        pre = 'backbone.convnext.0.'
        w = {k: v.float() for k, v in ref.w.items()}
        out, ln_only = torch.full((P, D), 7.0), torch.full((P, D), 7.0)
        two_f, lds = 2 * F_, -(-2 * F_ // 32) * 32
        Y = torch.cat([torch.linspace(-8.0, 8.0, P * F_).view(P, F_), torch.linspace(-20.0, 20.0, P * F_).view(F_, P).t()], 1)
        Y = Y.contiguous()
        S = torch.full((P, lds), 7.0)
        frames = torch.randn(P, L, generator=g)
        T = m.samples(max(lens))
        wave = torch.full((len(lens), 1, T), 7.0)
        wsq = (ref.w['head.istft.window'] ** 2).float()
        with _emulated(vocos_emu):
            native.vc_dwln(X, w[pre + 'dwconv.weight'][:, 0, :].t().contiguous(), w[pre + 'dwconv.bias'], w[pre + 'norm.weight'],
                           w[pre + 'norm.bias'], 1e-6, rowb0, out)
            native.vc_dwln(X, None, None, w['backbone.norm.weight'], w['backbone.norm.bias'], 1e-6, rowb0, ln_only)
            native.vc_polar(Y, F_, 100.0, rowb0, S)
            native.vc_ola(frames, wsq, utt, hop, m.trim(), wave)
        assert not out[~real].any() and not ln_only[~real].any() and not S[~real].any() and not S[:, two_f:].any()
        mag = torch.clamp(torch.exp(Y[:, :F_].double()), max=100.0)
        want_s = torch.stack([mag * torch.cos(Y[:, F_:].double()), mag * torch.sin(Y[:, F_:].double())], 2).view(P, two_f)
        assert (S[real][:, :two_f].double() - want_s[real]).abs().max() < 4e-7 * 100.0      # expf / sincosf: a few ulp of 100
        assert (mag[real] == 100.0).any() and (mag[real] < 1e-2).any()
        for b, (o, n) in enumerate(zip(offs, lens)):
            x = X[o:o + n].double().t()[None]
            y = torch.nn.functional.conv1d(x, ref.w[pre + 'dwconv.weight'], ref.w[pre + 'dwconv.bias'], padding=3, groups=D)
            want = vr.layer_norm(y, ref.w[pre + 'norm.weight'], ref.w[pre + 'norm.bias'])[0].t()
            assert (out[o:o + n].double() - want).abs().max() < 1e-5, name          # f32 sums of D terms on values of order 1
            want = vr.layer_norm(x, ref.w['backbone.norm.weight'], ref.w['backbone.norm.bias'])[0].t()
            assert (ln_only[o:o + n].double() - want).abs().max() < 1e-5, name
            fr = frames[o:o + n].double().t()[None]
            full = vr.overlap_add(fr, hop) / vr.overlap_add((ref.w['head.istft.window'] ** 2)[None, :, None].expand(1, L, n), hop)
            t = m.trim()
            want = full[0, t:full.shape[1] - t]
            assert want.numel() == m.samples(n)
            got = wave[b, 0]
            if want.numel():
                assert (got[:want.numel()].double() - want).abs().max() < 1e-5 * max(1.0, want.abs().max().item()), (name, b)
            assert not got[want.numel():].any()


# ---------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,msg", [(["--waveglow", "w.pt"], "give one"), (["--hifigan", "g.pt"], "give one"),
                                       (["--sigma", "0.5"], "draws no noise"), (["--denoise", "0.01"], "Denoiser")])
def test_cli_rejects_other_vocoders_options_with_vocos(extra, msg, capsys):
    from tacotron2_amd import vocode
    with pytest.raises(SystemExit) as e:
        vocode.main(["m.npy", "-o", "out", "--vocos", "v.pt"] + extra)
    assert e.value.code == 2 and msg in capsys.readouterr().err


def test_cli_accepts_vocos_and_checks_hop_and_mels_against_hparams(native_lib, tmp_path):
    from tacotron2_amd import vocode
    with pytest.raises(FileNotFoundError):                     # parsing passes; the mels are read before any GPU work
        vocode.main([str(tmp_path / "missing.npy"), "-o", str(tmp_path), "--vocos", "v.pt", "--precision", "bf16"])
    mel = str(tmp_path / "m.npy")
    np.save(mel, vr.make_mel(1, 6, 1)[0].numpy())
    ckpt = str(tmp_path / "v.pt")
    torch.save({'state_dict': vr.make_ref('odd', 1).state_dict()}, ckpt)          # 80 mels, but hop 32 against hparams' 256
    with pytest.raises(SystemExit, match="hop"):
        vocode.main([mel, "-o", str(tmp_path), "--vocos", ckpt])
    torch.save(vr.make_ref('small', 1).state_dict(), ckpt)                        # 20 mels against hparams' 80
    with pytest.raises(SystemExit, match="mel channels"):
        vocode.main([mel, "-o", str(tmp_path), "--vocos", ckpt, "--hparams", "hop_length=16"])
