"""The backward pass of the mel front end and the mel L1 loss without a GPU: the differentiable restatement
(tests/audio_grad_ref.py) against the oracle, the input margins of every case the GPU tests run, the models of the formulas of
csrc/audio_bwd.hip against float64 autograd of their forward pieces, that very source run on the host stand-in against the
models, and the host plumbing (shapes, refusals, kept state) in validate-only mode."""
import contextlib
import ctypes
import importlib.util
import os

import pytest
import torch

import audio_grad_ref as ar
import golden_util as gu
from oracle import audio_oracle as ao
from tacotron2_amd import audio, native


def _golden_signal():
    g = torch.load(os.path.join(gu.ROOT, "tests", "golden", "audio_demo.pt"), weights_only=False)
    return g["y"].reshape(1, -1)[:, :6000]


# ---- the restatement ----------------------------------------------------------------------------------------------------
def test_restatement_forward_is_the_oracle():
    """In float32 the restatement is the oracle's own sequence of torch calls (the guarded sqrt changes no value): equal
    bits.  In float64 it differs from it by float32 rounding only."""
    cases = [(ar.signal(k), ar.CASES[k][0]) for k in ar.CASES] + [(_golden_signal().double(), ar.DEFAULT)]
    for y, geom in cases:
        want = ao.mel_spectrogram(y.float(), **geom)
        assert torch.equal(ar.logmel(y.float(), geom), want)
        got = ar.logmel(y, geom)
        assert got.dtype == torch.float64 and (got - want.double()).abs().max().item() < 2e-5


def test_silent_bins_have_zero_gradient_in_the_restatement():
    y = ar.signal('B').clone()
    y[:, 1000:] = 0.0
    g = ar.grad_smooth(y, ar.DEFAULT, ar.loss_weights((1, 80, 9), 3))
    assert torch.isfinite(g).all() and g[:, :1000].abs().max() > 0


@pytest.mark.parametrize("name", sorted(ar.CASES))
def test_input_margins_of_the_gpu_cases(name):
    """Every float64 mel bin is far above the clamp, and every |log-mel - target| of the L1 cases at least 0.1: no precision
    puts a bin on the other side of either kink."""
    geom, B, T = ar.CASES[name]
    y = ar.signal(name)
    assert y.shape == (B, T) and y.abs().max() <= 1.0
    assert ar.mel(y, geom).min().item() >= ar.MIN_MEL
    lm = ar.logmel(y, geom)
    assert lm.shape == (B, geom['n_mel_channels'], T // geom['hop_length'] + 1)
    for seed in (12, 13):
        assert (lm - ar.l1_target(lm, seed)).abs().min().item() >= ar.MIN_DIFF


# ---- the formulas -------------------------------------------------------------------------------------------------------
def _pieces(name):
    """float64 intermediate images of a case in the product's layouts: spec (R, 2F), mag (R, F), mel rows (R, n_mel)."""
    geom, B, T = ar.CASES[name]
    L, hop = geom['filter_length'], geom['hop_length']
    fb, mb = ar.tables(geom)
    y = ar.signal(name)
    x = torch.nn.functional.pad(y.view(B, 1, 1, T), (L // 2, L // 2, 0, 0), mode='reflect').view(B, -1)
    n = T // hop + 1
    frames = torch.stack([x[b, j * hop:j * hop + L] for b in range(B) for j in range(n)])
    return geom, B, T, n, fb.view(-1, L), mb, frames


@pytest.mark.parametrize("name", ['A', 'C'])
def test_models_compose_to_the_autograd_gradient(name):
    geom, B, T, n, fb, mb, frames = _pieces(name)
    L, hop, Fb = geom['filter_length'], geom['hop_length'], geom['filter_length'] // 2 + 1
    spec = frames @ fb.t()
    mel_rows = torch.sqrt(spec[:, :Fb] ** 2 + spec[:, Fb:] ** 2) @ mb.t()
    r = ar.loss_weights((B, geom['n_mel_channels'], n), 5)
    d_mel = ar.log_bwd(r, mel_rows)
    d_spec = ar.magnitude_bwd(d_mel @ mb, spec, Fb, 2 * Fb)
    d_y = ar.frames_fold(d_spec @ fb, B, T, L, hop)
    want = ar.grad_smooth(ar.signal(name), geom, r)
    assert ((d_y - want).norm() / want.norm()).item() < 1e-12


def test_l1_model_is_the_autograd_gradient():
    g = torch.Generator().manual_seed(1)
    out = torch.randn(3, 5, 9, generator=g, dtype=torch.float64).requires_grad_(True)
    target = torch.randn(3, 5, 7, generator=g, dtype=torch.float64)
    lens = [7, 1, 3]
    loss = ar.l1_loss(out, target, lens)
    (loss * 0.7).backward()
    assert torch.equal(out.grad, ar.l1_bwd(out.detach(), target, lens, 0.7, 5 * sum(lens)))
    assert not out.grad[:, :, 7:].any() and not out.grad[1, :, 1:].any()


# ---- csrc/audio_bwd.hip on the host stand-in ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bwd_emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_audio_bwd_emu",
                                                  os.path.join(gu.ROOT, "tests", "hip_emu", "build_audio_bwd_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    emu = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("audio_bwd_emu"))))
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


def _near(got, want, tol):
    assert got.shape == want.shape
    assert (got.double() - want.double()).abs().max().item() <= tol * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("name", ['A', 'C'])
def test_emulated_kernels_equal_the_models(bwd_emu, name):
    geom, B, T, n, fb, mb, frames = _pieces(name)
    L, hop, Fb, n_mel = geom['filter_length'], geom['hop_length'], geom['filter_length'] // 2 + 1, geom['n_mel_channels']
    R, Kp = B * n, (2 * Fb + 31) // 32 * 32
    spec = (frames @ fb.t()).float()
    spec[0, 3] = spec[0, Fb + 3] = 0.0                                    # a bin of magnitude exactly 0
    mel_rows = (torch.sqrt(spec[:, :Fb].double() ** 2 + spec[:, Fb:].double() ** 2) @ mb.t()).float()
    mel_rows[1, 2], mel_rows[1, 3] = 1e-5, 0.5e-5                         # on the clamp (passes), below it (zero)
    g = torch.Generator().manual_seed(2)
    d_out = torch.randn(B, n_mel, n, generator=g)
    d_mag = torch.randn(R, (Fb + 15) // 16 * 16, generator=g)
    d_frames = torch.randn(R, L, generator=g)
    with _emulated(bwd_emu):
        d_mel = torch.full((R, n_mel), 7.0)
        native.mel_log_bwd(d_out, mel_rows, d_mel, 1e-5)
        d_spec = torch.full((R, Kp), 7.0)
        native.stft_magnitude_bwd(d_mag, spec, d_spec, Fb)
        d_y = torch.full((B, T), 7.0)
        native.stft_frames_fold(d_frames, d_y, hop, L // 2)
        d_y2 = torch.full((B, T), 7.0)
        native.stft_frames_fold(d_frames, d_y2, hop, L // 2)
        wide = torch.full((B, T + 3), 7.0)                                  # rows at a stride that forbids 16-byte stores
        native.stft_frames_fold(d_frames[:, :L], wide[:, :T], hop, L // 2)
    want = ar.log_bwd(d_out, mel_rows)
    _near(d_mel, want, 2e-7 * 1e5)                                          # quotients up to 1e5 x the gradient
    assert d_mel[1, 2] == d_out.permute(0, 2, 1).reshape(R, n_mel)[1, 2] / mel_rows[1, 2] and d_mel[1, 3] == 0.0
    _near(d_spec, ar.magnitude_bwd(d_mag, spec, Fb, Kp), 4e-7)              # the same float32 operations: a few last bits
    assert d_spec[0, 3] == 0.0 and d_spec[0, Fb + 3] == 0.0 and not d_spec[:, 2 * Fb:].any()
    _near(d_y, ar.frames_fold(d_frames.double(), B, T, L, hop), 1e-5)
    assert torch.equal(d_y, d_y2) and torch.equal(wide[:, :T], d_y) and (wide[:, T:] == 7.0).all()


def test_emulated_fold_sums_in_the_stated_order(bwd_emu):
    """T = L/2 + 1: both mirrors fold onto the same samples.  The kernel's float32 sum is the running sum over pad - t,
    pad + t, pad + 2 (T - 1) - t, frames ascending: equal bits with a float32 loop in that order."""
    L, hop, T = 32, 8, 17
    pad, n = L // 2, T // hop + 1
    d_frames = torch.randn(n, L, generator=torch.Generator().manual_seed(4))
    with _emulated(bwd_emu):
        d_y = torch.empty(1, T)
        native.stft_frames_fold(d_frames, d_y, hop, pad)
        for t in range(T):
            acc, seen = torch.zeros((), dtype=torch.float32), set()
            for q in (pad - t, pad + t, pad + 2 * (T - 1) - t):
                if q < 0 or q >= T + 2 * pad or q in seen:
                    continue
                seen.add(q)
                for j in range(n):
                    if j * hop <= q < j * hop + L:
                        acc = acc + d_frames[j, q - j * hop]
            assert d_y[0, t] == acc, t


def test_reflect_rule_is_the_one_the_fold_uses(native_lib):
    """The three positions the fold visits are exactly the padded positions that the forward's index rule maps onto t."""
    for T, pad in ((513, 512), (17, 16), (2125, 512), (1500, 256)):
        for t in (0, 1, pad // 2, pad, T - 1 - pad, T - 2, T - 1):
            if not 0 <= t < T:
                continue
            hits = sorted(q for q in range(T + 2 * pad) if native.reflect_index(q - pad, T) == t)
            cand = sorted({q for q in (pad - t, pad + t, pad + 2 * (T - 1) - t) if 0 <= q < T + 2 * pad})
            assert hits == cand, (T, pad, t)


def test_emulated_l1_kernels(bwd_emu):
    g = torch.Generator().manual_seed(6)
    B, n_mel, n, N = 3, 5, 70, 66
    out, target = torch.randn(B, n_mel, n, generator=g), torch.randn(B, n_mel, N, generator=g)
    target[0, 0, 0] = out[0, 0, 0]                                          # a zero difference: sign 0
    for lens in (None, [66, 1, 33]):
        count = n_mel * (B * N if lens is None else sum(lens))
        lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32)
        with _emulated(bwd_emu):
            slots = native.mel_l1_slots(B, n_mel, n)
            partial = torch.full((slots + 2,), 7.0)
            native.mel_l1_fwd(out, target, lens_t, count, partial)
            again = torch.full((slots + 2,), 7.0)
            native.mel_l1_fwd(out, target, lens_t, count, again)
            d_out = torch.full((B, n_mel, n), 7.0)
            native.mel_l1_bwd(out, target, lens_t, torch.tensor([0.7]), count, d_out)
        want = ar.l1_loss(out.double(), target.double(), lens).item()
        assert abs(partial[:slots].double().sum().item() - want) < 1e-6 * want
        assert torch.equal(partial, again) and (partial[slots:] == 7.0).all()
        assert torch.equal(d_out, ar.l1_bwd(out, target, lens, torch.tensor(0.7) / torch.tensor(float(count)), 1.0))
        assert d_out[0, 0, 0] == 0.0 and not d_out[:, :, N:].any()


# ---- host plumbing ---------------------------------------------------------------------------------------------------------
def _err(fn, *a, match):
    with pytest.raises(native.NativeError, match=match):
        fn(*a)


def test_entries_reject_bad_arguments(native_lib):
    native.set_validate_only(True)
    try:
        z = torch.zeros
        B, n, n_mel, Fb, L, hop = 2, 3, 8, 17, 32, 8
        T, R, Kp = 17, 2 * 3, 64
        native.mel_log_bwd(z(B, n_mel, n), z(R, n_mel), z(R, n_mel), 1e-5)
        _err(native.mel_log_bwd, z(B, n_mel, n), z(R, n_mel), z(R, n_mel), 0.0, match="clip")
        _err(native.mel_log_bwd, z(B, n_mel, n + 1), z(R, n_mel), z(R, n_mel), 1e-5, match="shape mismatch")
        m = z(R, n_mel)
        _err(native.mel_log_bwd, z(B, n_mel, n), m, m, 1e-5, match="must not be one of the inputs")
        native.stft_magnitude_bwd(z(R, 32), z(R, 2 * Fb), z(R, Kp), Fb)
        _err(native.stft_magnitude_bwd, z(R, 32), z(R, 2 * Fb), z(R, 2 * Fb - 1), Fb, match="shape mismatch")
        _err(native.stft_magnitude_bwd, z(R + 1, 32), z(R, 2 * Fb), z(R, Kp), Fb, match="shape mismatch")
        native.stft_frames_fold(z(R, L), z(B, T), hop, L // 2)
        _err(native.stft_frames_fold, z(R + 1, L), z(B, T), hop, L // 2, match="frame rows")
        _err(native.stft_frames_fold, z(R, L), z(B, T), hop, T, match="smaller than the signal")
        _err(native.stft_frames_fold, z(R, L), z(B, T), hop, 4, match="beyond the padded signal")
        out, tgt = z(B, n_mel, n), z(B, n_mel, 2)
        slots = native.mel_l1_slots(B, n_mel, n)
        native.mel_l1_fwd(out, tgt, None, B * n_mel * 2, z(slots))
        _err(native.mel_l1_fwd, out, z(B, n_mel, n + 1), None, 1, z(slots), match="more frames")
        _err(native.mel_l1_fwd, out, tgt, None, 0, z(slots), match="count")
        assert slots == 1 and native.mel_l1_slots(B, n_mel, 20000) == B * n_mel          # about 16k elements per slot
        _err(native.mel_l1_fwd, z(B, n_mel, 20000), tgt, None, 8, z(B * n_mel - 1), match="slots")
        _err(native.mel_l1_fwd, out, tgt, torch.zeros(B, dtype=torch.int64), 8, z(slots), match="int32")
        native.mel_l1_bwd(out, tgt, None, z(1), 8, z(B, n_mel, n))
        _err(native.mel_l1_bwd, out, tgt, None, z(2), 8, z(B, n_mel, n), match="g of 2")
        _err(native.mel_l1_bwd, out, tgt, None, z(1), 8, out, match="must not be one of the inputs")
        # an output that shares one element with an input is refused (byte ranges, not pointer equality); the neighbour is not
        buf, k = z(3 * R * n_mel), R * n_mel
        mel, d_out = buf[:k].view(R, n_mel), buf[2 * k:].view(B, n_mel, n)
        native.mel_log_bwd(d_out, mel, buf[k:2 * k].view(R, n_mel), 1e-5)
        _err(native.mel_log_bwd, d_out, mel, buf[k - 1:2 * k - 1].view(R, n_mel), 1e-5, match="must not be one of the inputs")
        _err(native.mel_log_bwd, d_out, mel, buf[k + 1:2 * k + 1].view(R, n_mel), 1e-5, match="must not be one of the inputs")
        buf, ks, kd = z(R * (2 * Fb + Kp + 32)), R * 2 * Fb, R * Kp
        spec, d_mag = buf[:ks].view(R, 2 * Fb), buf[ks + kd:].view(R, 32)
        native.stft_magnitude_bwd(d_mag, spec, buf[ks:ks + kd].view(R, Kp), Fb)
        _err(native.stft_magnitude_bwd, d_mag, spec, buf[ks - 1:ks + kd - 1].view(R, Kp), Fb, match="must not be one of the inputs")
        # d_mag's last row ends after F of its 32 floats: the first overlapping d_spec reaches into the element F - 1 of that row
        native.stft_magnitude_bwd(buf[:R * 32].view(R, 32), z(R, 2 * Fb), buf[(R - 1) * 32 + Fb:(R - 1) * 32 + Fb + kd].view(R, Kp), Fb)
        _err(native.stft_magnitude_bwd, buf[:R * 32].view(R, 32), z(R, 2 * Fb),
             buf[(R - 1) * 32 + Fb - 1:(R - 1) * 32 + Fb - 1 + kd].view(R, Kp), Fb, match="must not be one of the inputs")
        buf, k, kt = z(3 * B * n_mel * n), B * n_mel * n, B * n_mel * 2
        out, tgt = buf[:k].view(B, n_mel, n), buf[2 * k:2 * k + kt].view(B, n_mel, 2)
        native.mel_l1_bwd(out, tgt, None, z(1), 8, buf[k:2 * k].view(B, n_mel, n))
        _err(native.mel_l1_bwd, out, tgt, None, z(1), 8, buf[k - 1:2 * k - 1].view(B, n_mel, n), match="must not be one of the inputs")
        _err(native.mel_l1_bwd, out, tgt, None, z(1), 8, buf[k + 1:2 * k + 1].view(B, n_mel, n), match="must not be one of the inputs")
    finally:
        native.set_validate_only(False)


def test_autograd_surface_validate_only(native_lib, monkeypatch):
    """Shapes, launches and kept state of mel_spectrogram's and MelLoss's autograd functions; every entry's checks run."""
    native.set_validate_only(True)
    calls = []
    for fn in ('mel_log_bwd', 'stft_magnitude_bwd', 'stft_frames_fold', 'mel_l1_fwd', 'mel_l1_bwd', 'gemm', 'mel_log_compress'):
        real = getattr(native, fn)
        monkeypatch.setattr(native, fn, lambda *a, _f=fn, _r=real, **k: (calls.append((_f, k.get('fast'))), _r(*a, **k))[1])
    try:
        st = audio.TacotronSTFT()
        y = torch.zeros(2, 2125, dtype=torch.float64, requires_grad=True)
        assert not st.mel_spectrogram(y.detach()).requires_grad
        with torch.no_grad():
            assert not st.mel_spectrogram(y).requires_grad
        for prec, fast in (('fp32', 0), ('bf16x3', 1)):
            del calls[:]
            out = st.mel_spectrogram(y, check_range=False, precision=prec)
            assert out.requires_grad and tuple(out.shape) == (2, 80, 9) and out.dtype == torch.float32
            spec, mel_rows = out.grad_fn.kept
            assert spec.numel() + mel_rows.numel() == st.kept_state_floats(2, 2125) == 18 * (1026 + 80)
            assert [c for c, _ in calls] == ['gemm', 'gemm', 'mel_log_compress']
            del calls[:]
            out.sum().backward()
            assert calls == [('mel_log_bwd', None), ('gemm', fast), ('stft_magnitude_bwd', None), ('gemm', fast),
                             ('stft_frames_fold', None)]
            assert y.grad.shape == y.shape
            with pytest.raises(RuntimeError, match="already run"):
                out.sum().backward()
        with pytest.raises(ValueError, match="precision"):
            st.mel_spectrogram(y, precision='bf16')
        assert 'fbt' in st.stft_fn.bwd_tables('cpu') and tuple(st.stft_fn.bwd_tables('cpu')['fbt'].shape) == (1024, 1056)
        assert tuple(st.mel_basis_t('cpu').shape) == (528, 80)
        assert 'fbt' not in dict(st.named_buffers()) and len(dict(st.named_buffers())) == 3

        ml = audio.MelLoss(st)
        a = torch.zeros(2, 1, 2125, requires_grad=True)
        del calls[:]
        loss = ml(a, torch.zeros(2, 80, 8), lengths=torch.tensor([8, 3]), precision='bf16x3')
        assert loss.dim() == 0 and loss.requires_grad
        loss.backward()
        assert a.grad.shape == a.shape
        assert [c for c, _ in calls] == ['gemm', 'gemm', 'mel_log_compress', 'mel_l1_fwd', 'mel_log_compress', 'mel_l1_bwd',
                                         'mel_log_bwd', 'gemm', 'stft_magnitude_bwd', 'gemm', 'stft_frames_fold']
        for bad, match in (((torch.zeros(2, 2, 2125), torch.zeros(2, 80, 8)), r"\(B, T\) or \(B, 1, T\)"),
                           ((torch.zeros(2, 2125), torch.zeros(2, 79, 8)), r"target log-mels"),
                           ((torch.zeros(2, 2125), torch.zeros(3, 80, 8)), r"target log-mels"),
                           ((torch.zeros(2, 2125), torch.zeros(2, 80, 10)), r"10 frames, 2125 samples give 9")):
            with pytest.raises(ValueError, match=match):
                ml(*bad)
        for lens in ([8], [0, 8], [9, 8]):
            with pytest.raises(ValueError, match="lengths"):
                ml(torch.zeros(2, 2125), torch.zeros(2, 80, 8), lengths=lens)
        with pytest.raises(TypeError):
            audio.MelLoss(st.stft_fn)
    finally:
        native.set_validate_only(False)
    if not torch.cuda.is_available():
        with pytest.raises(native.NativeError, match="move the module to the MI355X first"):
            audio.MelLoss(audio.TacotronSTFT())(torch.zeros(1, 2125), torch.zeros(1, 80, 8))
