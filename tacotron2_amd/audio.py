"""wav -> log-mel on the MI355X.

Interface of the reference's ``layers.TacotronSTFT`` (reference layers.py:42-80) and the forward
half of ``stft.STFT`` (reference stft.py:42-105): ``TacotronSTFT(filter_length, hop_length,
win_length, n_mel_channels, sampling_rate, mel_fmin, mel_fmax).mel_spectrogram(y)`` with ``y``
(B, T) in [-1, 1] returns (B, n_mel_channels, T // hop + 1) log-mels, buffers ``mel_basis`` and
``stft_fn.forward_basis`` as in the reference.

Arithmetic (same as the reference, different schedule):
  1. reflect-pad by filter_length/2 on both sides                       (csrc/audio.hip)
  2. spec = frames . forward_basis^T on the exact-f32 MFMA GEMM; the frame matrix is never built:
     the padded signal is the A operand with row stride ``hop`` (< K, rows overlap)   (gemm.hip)
  3. magnitude sqrt(re^2 + im^2)                                        (csrc/audio.hip)
  4. mel = mag . mel_basis^T                                            (gemm.hip)
  5. log(clamp(mel, 1e-5)) and the transpose to (B, n_mel, frames)      (csrc/audio.hip)
No torch arithmetic touches the samples; torch allocates the buffers.  There is no CPU path.

The mel filterbank is librosa 0.6.0's ``filters.mel(sr, n_fft, n_mels, fmin, fmax)`` (htk=False,
norm=1: Slaney's Auditory-Toolbox scale, area-normalised triangles), which the reference calls at
layers.py:50-51; librosa is not vendored in the reference and not installed here, so the published
algorithm is restated in ``mel_filterbank`` (parity for this table is unpinned by any reference
artefact; the STFT/magnitude/log part is pinned against the reference's own stft.py run on CPU,
tests/golden/make_golden_audio.py).

mel -> wav (Griffin-Lim, reference audio_processing.py:59-76 and stft.py:77-141), also on the GPU:
``STFT.transform`` returns (magnitude, phase), ``STFT.inverse`` / ``STFT.forward`` invert it, ``griffin_lim``
iterates the two over a ragged batch, ``TacotronSTFT.mel_to_magnitude`` / ``TacotronSTFT.vocode`` start from
log-mels.  One iteration on the whole batch is four launches on one stream (csrc/vocoder.hip, gemm.hip):
  1. frames = rec . IB^T on the GEMM (IB = the reference's windowed pinv(scale * fourier_basis), built lazily in
     float64 and cached per geometry; not a module buffer, so building a TacotronSTFT stays cheap)
  2. overlap-add: ascending frame order, the float32 window sum-square rebuilt on the fly, / where > tiny, * L/hop,
     written straight into the reflect-padded input of the next forward transform
  3. spec = padded (lda = hop) . FB^T on the GEMM, exactly as the mel path
  4. projection rec = S * z / |z| (no angle, cos or sin inside the loop)
Ragged batches run in one packed frame space (utterance b owns n_b + ceil(L/hop) - 1 consecutive rows), so the GEMMs
cover sum(n_b + 3) rows at L = 1024, hop = 256, not B * n_max.  The mel inversion is the clamped pseudo-inverse
max(pinv(mel_basis) . exp(mel), 0) (the reference gives no recipe).

Steps 1 and 2 are ``STFT.frame_spectra`` for every transform of this file (the mel path, ``STFT.transform``, the STFT loss), and
``STFT.spectrum_backward`` (d_frames = d_spec . forward_basis, overlap-add with the reflect fold) is the tail of every backward.

The way back (csrc/audio_bwd.hip): ``mel_spectrogram`` of a signal that requires grad returns the same
bits with a ``grad_fn``; it keeps the spectrum and the mel rows and its backward is five launches (log-compress backward,
d_mag = d_mel . mel_basis, magnitude backward, d_frames = d_spec . forward_basis, overlap-add with the reflect fold).
``MelLoss(stft)(audio, target_mel, lengths)`` is the masked mean |log-mel(audio) - target| as one autograd function from the
samples to the scalar: the term a vocoder is fine-tuned on (``tacotron2_amd.vocos_train``).  Two subgradients are definitions:
the clamp passes the gradient where mel >= clip (torch's rule), and a bin of magnitude exactly 0 gets gradient 0 (torch's
sqrt gives NaN there).

``MultiResolutionSTFTLoss()(audio, target_audio, lengths)`` is the spectral-convergence plus log-magnitude loss over several STFT
geometries (csrc/stft_loss.hip), again one autograd function from the samples to the scalar: fused row
kernels straight off the two spectra, fixed-order float64 partial sums, no atomics and no host synchronisation.

``Resample(orig_freq, new_freq)(x, lengths)`` / ``resample(x, orig_freq, new_freq, lengths)`` convert the sampling rate
(csrc/resample.hip): band-limited sinc interpolation with a Hann window as a polyphase gather, its adjoint as
a gather of the same shape, one autograd function, ragged batches equal to their utterances alone bit for bit.

``MelCepstralDistortion()(mel_a, mel_b, len_a, len_b)`` scores two log-mels of different lengths (csrc/dtw.hip, DESIGN.md section
16): ``mel_cepstrum`` (orthonormal DCT-II without c0), ``dtw`` (one workgroup per pair, fixed tie rule, path length carried with
the cost, the path itself on request), MCD in dB per pair.  Evaluation only: no gradients.
"""
import os

import numpy as np
import torch

from . import native as nv
from .vocoder import host_lengths

_F_SP = 200.0 / 3.0                  # Slaney: linear below 1 kHz, 200/3 Hz per mel
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP   # = 15
_LOGSTEP = np.log(6.4) / 27.0        # log-spaced above: 27 mels per factor 6.4


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    lin = f / _F_SP
    log = _MIN_LOG_MEL + np.log(np.maximum(f, _MIN_LOG_HZ) / _MIN_LOG_HZ) / _LOGSTEP
    return np.where(f >= _MIN_LOG_HZ, log, lin)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    lin = _F_SP * m
    log = _MIN_LOG_HZ * np.exp(_LOGSTEP * (np.maximum(m, _MIN_LOG_MEL) - _MIN_LOG_MEL))
    return np.where(m >= _MIN_LOG_MEL, log, lin)


def mel_filterbank(sr, n_fft, n_mels=128, fmin=0.0, fmax=None):
    """(n_mels, 1 + n_fft//2) float64 triangular filters, Slaney scale, each scaled by
    2 / (its band width in Hz) — librosa 0.6.0 ``filters.mel`` with its defaults."""
    if fmax is None:
        fmax = sr / 2.0
    n_bins = 1 + n_fft // 2
    bin_hz = np.linspace(0.0, sr / 2.0, n_bins)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    width = np.diff(edges)
    dist = edges[:, None] - bin_hz[None, :]                 # (n_mels+2, n_bins)
    rising = -dist[:-2] / width[:-1, None]
    falling = dist[2:] / width[1:, None]
    tri = np.maximum(0.0, np.minimum(rising, falling))
    return tri * (2.0 / (edges[2:] - edges[:-2]))[:, None]


def fourier_basis(filter_length, win_length, window='hann'):
    """(2F, filter_length) float32: rows [cos | -sin](2 pi f k / L), F = L/2 + 1, each multiplied in float32
    by the periodic window zero-padded (centred) to filter_length — what stft.py:53-70 registers."""
    L = int(filter_length)
    if win_length > L:
        raise AssertionError("filter_length must be >= win_length")
    F = L // 2 + 1
    k = np.arange(L, dtype=np.float64)
    ang = 2.0 * np.pi * np.outer(np.arange(F, dtype=np.float64), k) / L
    basis = np.vstack([np.cos(ang), -np.sin(ang)]).astype(np.float32)
    if window is not None:
        if window != 'hann':
            raise ValueError("only the periodic hann window of the reference is built in")
        n = np.arange(win_length, dtype=np.float64)
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)
        lpad = (L - win_length) // 2
        wfull = np.zeros(L, dtype=np.float64)
        wfull[lpad:lpad + win_length] = w
        basis = basis * wfull.astype(np.float32)[None, :]
    return basis


def _pad_center(data, size):
    lpad = (size - data.shape[-1]) // 2
    return np.pad(data, (lpad, size - data.shape[-1] - lpad), mode='constant')


def _squared_window(window, win_length, n_fft):
    """float64 squared window zero-padded (centred) to n_fft: ``win_sq`` of the reference's window_sumsquare."""
    from scipy.signal import get_window
    return _pad_center(get_window(window, win_length, fftbins=True) ** 2, n_fft)


def window_sumsquare(window, n_frames, hop_length=200, win_length=800, n_fft=800, dtype=np.float32, norm=None):
    """Sum-square envelope of the window at this hop (reference audio_processing.py:7-51, librosa 0.6), on the host.
    Only ``norm=None`` (what the reference's callers use) is supported."""
    if norm is not None:
        raise ValueError("window_sumsquare: only norm=None is supported")
    if win_length is None:
        win_length = n_fft
    n = n_fft + hop_length * (n_frames - 1)
    x = np.zeros(n, dtype=dtype)
    win_sq = _squared_window(window, win_length, n_fft)
    for i in range(n_frames):
        sample = i * hop_length
        x[sample:min(n, sample + n_fft)] += win_sq[:max(0, min(n_fft, n - sample))]
    return x


def dynamic_range_decompression(x, C=1):
    """exp(x) / C (reference audio_processing.py:87-93)."""
    return torch.exp(x) / C


_INVERSE_BASES = {}


def inverse_basis(filter_length, hop_length, win_length, window='hann'):
    """(2F, filter_length) float32: the reference's ``inverse_basis`` (stft.py:57-70): float32(pinv(L/hop * [Re; Im]
    fft(eye(L))[:F]).T) times the float32 window.  pinv of a 1026 x 1024 float64 matrix takes about a second on a CPU:
    built on first use and cached per geometry (read-only array)."""
    key = (int(filter_length), int(hop_length), int(win_length), window)
    ib = _INVERSE_BASES.get(key)
    if ib is None:
        L = key[0]
        if win_length > L:
            raise AssertionError("filter_length must be >= win_length")
        from scipy.signal import get_window
        cutoff = L // 2 + 1
        fb = np.fft.fft(np.eye(L))
        fb = np.vstack([np.real(fb[:cutoff, :]), np.imag(fb[:cutoff, :])])
        ib = np.linalg.pinv((L / hop_length) * fb).T.astype(np.float32)
        if window is not None:
            ib = ib * _pad_center(get_window(window, win_length, fftbins=True), L).astype(np.float32)[None, :]
        ib = np.ascontiguousarray(ib, dtype=np.float32)
        ib.setflags(write=False)
        _INVERSE_BASES[key] = ib
    return ib


def packed_rows(lengths, filter_length=1024, hop_length=256):
    """Rows of the packed frame space of a ragged batch: sum(n_b + ceil(L/hop) - 1)."""
    c = -(-int(filter_length) // int(hop_length))
    return int(sum(int(n) + c - 1 for n in lengths))


_PRECISIONS = {'fp32': 0, 'bf16x3': 1}


def _precision(precision):
    if precision not in _PRECISIONS:
        raise ValueError("precision must be one of %s, got %r" % (sorted(_PRECISIONS), precision))
    return _PRECISIONS[precision]


def _require_device(t, dry_run=True):
    """The modules of this file have no CPU path; validate-only mode passes when ``dry_run``."""
    if not t.is_cuda and not (dry_run and nv.validate_only()):
        raise nv.NativeError("tacotron2_amd.audio: move the module to the MI355X first (.cuda()); there is no CPU path")


def _device_signal(y, like):
    if y.dim() != 2:
        raise ValueError("expected (B, T) samples, got shape %s" % (tuple(y.shape),))
    _require_device(like)
    return y.detach().to(device=like.device, dtype=torch.float32).contiguous()


def _squeeze_channel(x):
    """(B, 1, T) -> (B, T); anything else as it is."""
    return x.reshape(x.shape[0], x.shape[2]) if x.dim() == 3 and x.shape[1] == 1 else x


def _lengths(lengths, B, hi, who="", full=None):
    """``vocoder.host_lengths`` with the count checked and, where ``hi`` is given, the range [1, hi]; None stays None unless
    ``full`` is given.  ``who`` prefixes the error text."""
    if lengths is None and full is None:
        return None
    lens = host_lengths(lengths, B, full)
    if len(lens) != B:
        raise ValueError("%s%d lengths for a batch of %d" % (who, len(lens), B))
    if hi is not None and (min(lens) < 1 or max(lens) > hi):
        raise ValueError("%slengths must lie in [1, %d], got %s" % (who, hi, lens))
    return lens


def _per_device(cache, name, device, build):
    """``build(device)`` once per (name, device): the tables that are plain attributes, not buffers, built on first use."""
    key = (name, torch.device(device))
    if key not in cache:
        cache[key] = build(key[1])
    return cache[key]


def _take_kept(ctx, who):
    """The state an autograd function kept for its backward, taken and freed."""
    kept, ctx.kept = ctx.kept, None
    if kept is None:
        raise RuntimeError("%s: backward was already run; the kept state is freed by the first one" % who)
    return kept


class STFT(torch.nn.Module):
    """reference stft.py:42-141 on the GPU: forward transform (magnitude, phase), inverse, reconstruction."""

    def __init__(self, filter_length=800, hop_length=200, win_length=800, window='hann'):
        super().__init__()
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        self.cutoff = filter_length // 2 + 1
        basis = torch.from_numpy(fourier_basis(filter_length, win_length, window))
        self.register_buffer('forward_basis', basis[:, None, :].contiguous())      # (2F, 1, L) like the reference
        self.Fpad = (self.cutoff + 15) // 16 * 16       # bins rounded up to the 16-wide column tiles of the row kernels
        self._lazy = {}                 # per device: the tables below (plain attributes, not buffers)

    def gl_tables(self, device):
        """Device tables of the inverse / Griffin-Lim path, built on first use: ``fbi`` (2F, L) forward basis with re/im
        rows interleaved, ``ibt`` (L, 2 Fpad) inverse basis transposed with interleaved columns (zero beyond 2F), ``wsq``
        (L,) float64 squared window."""
        def build(device):
            L, F = self.filter_length, self.cutoff
            fb = self.forward_basis.view(2 * F, L).to(device)
            perm = torch.stack([torch.arange(F), torch.arange(F) + F], 1).reshape(-1).to(device)
            ib = inverse_basis(L, self.hop_length, self.win_length, self.window)
            ibt = np.zeros((L, 2 * self.Fpad), dtype=np.float32)
            ibt[:, 0:2 * F:2] = ib[:F].T
            ibt[:, 1:2 * F:2] = ib[F:].T
            wsq = _squared_window(self.window, self.win_length, L) if self.window is not None else np.ones(L)
            return {"fbi": fb.index_select(0, perm).contiguous(), "ibt": torch.from_numpy(ibt).to(device),
                    "wsq": torch.from_numpy(np.ascontiguousarray(wsq, dtype=np.float64)).to(device)}
        return _per_device(self._lazy, 'gl', device, build)

    def bwd_tables(self, device):
        """Device table of the backward of the forward transform, built on first use: ``fbt`` (L, Kp) = forward_basis
        transposed, Kp = 2F rounded up to the 32-deep k-steps of the split-bf16 GEMM, zero columns beyond 2F (the B operand of
        d_frames = d_spec . forward_basis)."""
        def build(device):
            L, F = self.filter_length, self.cutoff
            Kp = (2 * F + 31) // 32 * 32
            fbt = torch.zeros(L, Kp, dtype=torch.float32, device=device)
            fbt[:, :2 * F] = self.forward_basis.view(2 * F, L).to(device).t()
            return {"fbt": fbt, "Kp": Kp}
        return _per_device(self._lazy, 'bwd', device, build)

    def frame_spectra(self, signals, basis, width):
        """The front end of every transform here: ``signals``, a list of (B, T) device float32 signals of equal T, each
        reflect-padded by L/2 into one buffer of rows of (T + L + 3) // 4 * 4 floats, then ONE GEMM over all of them,
        spec = frames . basis^T with batch = len(signals) B.  The frame matrix is never built: the A operand is the padded
        signal at row stride ``hop`` (rows overlap).  ``basis`` (2F, L) is ``forward_basis`` (rows [re | im]) or the
        interleaved ``fbi``; ``width`` >= 2F is the row width of the result.  -> (spec (len(signals) B n, width), n)."""
        B, T = signals[0].shape
        L, hop, F, dev = self.filter_length, self.hop_length, self.cutoff, signals[0].device
        if T <= L // 2:
            raise ValueError("signal of %d samples is too short to reflect-pad by %d" % (T, L // 2))
        n, batch = T // hop + 1, len(signals) * B
        ldo = (T + L + 3) // 4 * 4
        padded = torch.empty(batch, ldo, dtype=torch.float32, device=dev)
        for i, sig in enumerate(signals):
            nv.reflect_pad(sig, padded[i * B:(i + 1) * B], L // 2)
        spec = torch.empty(batch * n, width, dtype=torch.float32, device=dev)
        frames0 = padded.as_strided((n, L), (hop, 1))                              # utterance 0; rows overlap
        nv.gemm(spec[:n, :2 * F], frames0, basis, batch=batch, strides=(ldo, 0, n * width))
        return spec, n

    def spectrum_backward(self, d_spec, B, T, fast, out=None):
        """The tail of every backward here: d_y (B, T) from d_spec (B n, Kp) rows [d_re | d_im | 0], d_frames = d_spec .
        forward_basis on the GEMM, then the overlap-add with the fold of the reflect padding, into ``out`` when given."""
        L = self.filter_length
        d_frames = torch.empty(d_spec.shape[0], L, dtype=torch.float32, device=d_spec.device)
        nv.gemm(d_frames, d_spec, self.bwd_tables(d_spec.device)["fbt"], fast=fast)
        d_y = torch.empty(B, T, dtype=torch.float32, device=d_spec.device) if out is None else out
        nv.stft_frames_fold(d_frames, d_y, self.hop_length, L // 2)
        return d_y

    def magnitude_rows(self, y):
        """y (B, T) device f32 -> (mag (B*n, Fpad) with zero columns beyond F, n)."""
        mag, _, n = self._magnitude_spec_rows(y)
        return mag, n

    def _magnitude_spec_rows(self, y):
        """``magnitude_rows`` with the spectrum it came from: (mag, spec (B*n, 2F) rows [re | im], n)."""
        F = self.cutoff
        spec, n = self.frame_spectra([y], self.forward_basis.view(2 * F, self.filter_length), 2 * F)
        mag = torch.empty(spec.shape[0], self.Fpad, dtype=torch.float32, device=y.device)
        nv.stft_magnitude(spec, mag, F)
        return mag, spec, n

    def transform_magnitude(self, y):
        """(B, F, n) magnitudes, the first return value of the reference's ``transform``."""
        y = _device_signal(y, self.forward_basis)
        mag, n = self.magnitude_rows(y)
        out = torch.empty(y.shape[0], self.cutoff, n, dtype=torch.float32, device=y.device)
        nv.transpose(out.view(-1, n)[:self.cutoff], mag[:n, :self.cutoff], batch=y.shape[0],
                     sstride=n * mag.shape[1], dstride=self.cutoff * n)
        return out


    def transform(self, input_data):
        """(magnitude, phase), each (B, F, n): reference stft.py:77-105 (phase = atan2(im, re))."""
        y = _device_signal(input_data, self.forward_basis)
        spec, n = self.frame_spectra([y], self.gl_tables(y.device)["fbi"], 2 * self.Fpad)
        B, F = y.shape[0], self.cutoff
        mag = torch.empty(B, F, n, dtype=torch.float32, device=y.device)
        phase = torch.empty(B, F, n, dtype=torch.float32, device=y.device)
        nv.stft_polar(spec, B, n, F, mag, phase)
        self.num_samples = y.shape[1]
        return mag, phase

    def inverse(self, magnitude, phase):
        """(B, 1, (n-1) hop) signal from (B, F, n) magnitude and phase: reference stft.py:107-141."""
        out = _GriffinLim(self, magnitude, phase, None, 'fp32').run(0)
        return out.unsqueeze(1)

    def forward(self, input_data):
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)


class _GriffinLim:
    """One Griffin-Lim call over a ragged batch in the packed frame space.  Every buffer is allocated here, once; the
    iteration loop (run) issues four launches per iteration and no allocation, copy or synchronisation."""

    def __init__(self, stft, magnitudes, angles, lengths, precision):
        self.fast = _precision(precision)
        _require_device(stft.forward_basis)
        dev = stft.forward_basis.device
        L, hop, F = stft.filter_length, stft.hop_length, stft.cutoff
        mag = magnitudes.detach().to(device=dev, dtype=torch.float32).contiguous()
        if mag.dim() != 3 or mag.shape[1] != F:
            raise ValueError("expected (B, %d, n) magnitudes, got shape %s" % (F, tuple(mag.shape)))
        B, _, n = mag.shape
        lens = _lengths(lengths, B, n, full=n)
        ph = None
        if angles is not None:
            ph = torch.as_tensor(angles).detach().to(device=dev, dtype=torch.float32).contiguous()
            if tuple(ph.shape) != tuple(mag.shape):
                raise ValueError("angles %s do not match the magnitudes %s" % (tuple(ph.shape), tuple(mag.shape)))
        tab, Fp = stft.gl_tables(dev), stft.Fpad
        c = -(-L // hop)
        rows = np.asarray(lens, dtype=np.int64) + c - 1
        row0 = np.concatenate([[0], np.cumsum(rows)])
        R = int(row0[-1])
        plan = np.concatenate([row0, lens, np.repeat(np.arange(B), rows)]).astype(np.int32)
        self.stft, self.tab, self.B, self.R, self.F, self.Fp, self.L, self.hop = stft, tab, B, R, F, Fp, L, hop
        self.lens = nv._host_ints(lens)
        self.T = (max(lens) - 1) * hop
        self.plan = torch.from_numpy(plan).to(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.S = torch.empty(R, Fp, **f32)
        self.rec = torch.empty(R, 2 * Fp, **f32)
        self.frames = torch.empty(R, L, **f32)
        self.out = torch.empty(B, max(self.T, 1), **f32)
        self.mag, self.ph = mag, ph
        self.scale = float(L) / hop
        self.padded = self.spec = None

    def _inverse_frames(self):
        nv.gemm(self.frames, self.rec, self.tab["ibt"], fast=self.fast)

    def run(self, n_iters):
        lens, plan, R, L, hop, F, Fp = self.lens, self.plan, self.R, self.L, self.hop, self.F, self.Fp
        nv.gl_rect(self.mag, self.ph, plan, lens, R, L, hop, F, Fp, self.S, self.rec)
        if n_iters > 0:
            P = (R * hop + L + 3) // 4 * 4
            self.padded = torch.empty(P, dtype=torch.float32, device=self.frames.device)
            self.spec = torch.empty(R, 2 * Fp, dtype=torch.float32, device=self.frames.device)
            view = self.padded.as_strided((R, L), (hop, 1))
            spec_n = self.spec[:, :2 * F]
            fbi, wsq = self.tab["fbi"], self.tab["wsq"]
            for _ in range(n_iters):
                self._inverse_frames()
                nv.gl_overlap_add(self.frames, wsq, plan, lens, R, L, hop, self.scale, self.padded, 0)
                nv.gemm(spec_n, view, fbi, fast=self.fast)
                nv.gl_project(self.spec, self.S, plan, lens, R, L, hop, F, Fp, self.rec)
        self._inverse_frames()
        if self.T == 0:
            return self.out[:, :0]
        nv.gl_overlap_add(self.frames, self.tab["wsq"], plan, lens, R, L, hop, self.scale, self.out, 1)
        return self.out


def griffin_lim(magnitudes, stft_fn, n_iters=30, angles=None, lengths=None, precision='fp32'):
    """Reference audio_processing.py:59-76 on the GPU, over a ragged batch.

    magnitudes (B, F, n); stft_fn: this module's ``STFT`` (e.g. ``TacotronSTFT.stft_fn``).  ``angles`` (B, F, n) are the
    initial phases; when None they are drawn exactly as the reference draws them,
    ``np.angle(np.exp(2j pi np.random.rand(B, F, n))).astype(float32)``, so ``np.random.seed(s)`` gives the reference's
    start.  ``lengths`` (B ints): utterance b uses its first n_b frames only, and its output is the signal of those
    alone.  Returns (B, (max n_b - 1) hop) on the GPU, zero beyond each (n_b - 1) hop.  ``precision``: 'fp32' (exact f32
    GEMMs) or 'bf16x3' (split-bf16 GEMMs)."""
    if not isinstance(stft_fn, STFT):
        raise TypeError("griffin_lim needs a tacotron2_amd.audio.STFT (e.g. TacotronSTFT.stft_fn)")
    if angles is None:
        angles = np.angle(np.exp(2j * np.pi * np.random.rand(*magnitudes.size())))
        angles = torch.from_numpy(angles.astype(np.float32))
    return _GriffinLim(stft_fn, magnitudes, angles, lengths, precision).run(int(n_iters))


class TacotronSTFT(torch.nn.Module):
    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80,
                 sampling_rate=22050, mel_fmin=0.0, mel_fmax=8000.0):
        super().__init__()
        self.n_mel_channels = n_mel_channels
        self.sampling_rate = sampling_rate
        self.stft_fn = STFT(filter_length, hop_length, win_length)
        fb = mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)
        self.register_buffer('mel_basis', torch.from_numpy(fb).float())
        padded = torch.zeros(n_mel_channels, self.stft_fn.Fpad, dtype=torch.float32)
        padded[:, :self.stft_fn.cutoff] = self.mel_basis
        self.register_buffer('_mel_basis_padded', padded, persistent=False)
        self._lazy = {}                 # per device: mel_pinv and mel_basis_t, built on first use (not buffers)
        self.clip_val = 1e-5
        if torch.cuda.is_available():
            self.cuda()

    def spectral_normalize(self, magnitudes):
        """log(clamp(x, 1e-5)) (reference audio_processing.py:78-84) — elementwise convenience for callers
        outside the mel path; ``mel_spectrogram`` fuses it into its last kernel."""
        return torch.log(torch.clamp(magnitudes, min=self.clip_val))

    def spectral_de_normalize(self, magnitudes):
        return torch.exp(magnitudes)

    def mel_pinv(self, device):
        """(F, n_mel) float32 pseudo-inverse of the mel filterbank (float64 pinv of the float32 ``mel_basis``), built on
        first use (not a buffer)."""
        return _per_device(self._lazy, 'pinv', device, lambda d: torch.from_numpy(
            np.linalg.pinv(self.mel_basis.cpu().double().numpy()).astype(np.float32)).to(d))

    def mel_to_magnitude(self, mel, lengths=None):
        """Log-mel (B, n_mel, n) -> linear magnitudes (B, F, n) = max(pinv(mel_basis) . exp(mel), 0), zero beyond
        ``lengths``.  The reference has no recipe for this step; the clamped pseudo-inverse is the least-squares
        inverse of the filterbank.  fp16 / bf16 mels are cast to float32."""
        if mel.dim() != 3 or mel.shape[1] != self.n_mel_channels:
            raise ValueError("expected (B, %d, n) log-mels, got shape %s" % (self.n_mel_channels, tuple(mel.shape)))
        _require_device(self.mel_basis, dry_run=False)
        dev = self.mel_basis.device
        mel = mel.detach().to(device=dev, dtype=torch.float32).contiguous()
        B, n_mel, n = mel.shape
        F, Fp = self.stft_fn.cutoff, self.stft_fn.Fpad
        lens = _lengths(lengths, B, None)
        lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev)
        ldk = (n_mel + 3) // 4 * 4
        rows = torch.empty(B * n, ldk, dtype=torch.float32, device=dev)
        nv.mel_decompress(mel, rows, lens, lens_dev)
        lin = torch.empty(B * n, Fp, dtype=torch.float32, device=dev)
        nv.gemm(lin[:, :F], rows[:, :n_mel], self.mel_pinv(dev), act=1)
        out = torch.empty(B, F, n, dtype=torch.float32, device=dev)
        nv.transpose(out.view(-1, n)[:F], lin[:n, :F], batch=B, sstride=n * Fp, dstride=F * n)
        return out

    def vocode(self, mel, lengths=None, n_iters=30, precision='fp32', angles=None):
        """Log-mel (B, n_mel, n) -> waveform (B, (max n_b - 1) hop) in [-1, 1]-ish units on the GPU: mel_to_magnitude,
        then ``griffin_lim`` (initial angles drawn like the reference's when ``angles`` is None)."""
        mag = self.mel_to_magnitude(mel, lengths)
        return griffin_lim(mag, self.stft_fn, n_iters=n_iters, angles=angles, lengths=lengths, precision=precision)

    def mel_basis_t(self, device):
        """(Fpad, n_mel) float32: the zero-padded filterbank transposed, the B operand of d_mag = d_mel . mel_basis; built on
        first use (not a buffer)."""
        return _per_device(self._lazy, 'basis_t', device, lambda d: self._mel_basis_padded.to(d).t().contiguous())

    def _check_range(self, y):
        lo, hi = (float(v) for v in torch.stack(torch.aminmax(y)).tolist())
        if lo < -1.0 or hi > 1.0:
            raise AssertionError("samples must lie in [-1, 1] (got [%g, %g]); divide by max_wav_value" % (lo, hi))

    def _mel_forward(self, y):
        """The launches of ``mel_spectrogram`` on device samples y (B, T) -> (log-mels, spec rows, mel rows)."""
        mag, spec, n = self.stft_fn._magnitude_spec_rows(y)
        B = y.shape[0]
        mel_rows = torch.empty(B * n, self.n_mel_channels, dtype=torch.float32, device=y.device)
        nv.gemm(mel_rows, mag, self._mel_basis_padded)
        out = torch.empty(B, self.n_mel_channels, n, dtype=torch.float32, device=y.device)
        nv.mel_log_compress(mel_rows, out, self.clip_val)
        return out, spec, mel_rows

    def kept_state_floats(self, B, T):
        """Floats kept between the forward and the backward of ``mel_spectrogram`` / ``MelLoss`` for (B, T) samples: the
        spectrum (B n, 2F) and the mel rows (B n, n_mel)."""
        n = T // self.stft_fn.hop_length + 1
        return B * n * (2 * self.stft_fn.cutoff + self.n_mel_channels)

    def _mel_backward(self, d_out, spec, mel_rows, B, T, fast):
        """d_y (B, T) float32 from d_out (B, n_mel, n) and the kept spectrum and mel rows: five launches."""
        st = self.stft_fn
        dev, R = spec.device, spec.shape[0]
        f32 = dict(dtype=torch.float32, device=dev)
        d_mel = torch.empty(R, self.n_mel_channels, **f32)
        nv.mel_log_bwd(d_out, mel_rows, d_mel, self.clip_val)
        d_mag = torch.empty(R, st.Fpad, **f32)
        nv.gemm(d_mag, d_mel, self.mel_basis_t(dev), fast=fast)
        d_spec = torch.empty(R, st.bwd_tables(dev)["Kp"], **f32)
        nv.stft_magnitude_bwd(d_mag, spec, d_spec, st.cutoff)
        return st.spectrum_backward(d_spec, B, T, fast)

    def mel_spectrogram(self, y, check_range=True, precision='fp32'):
        """y (B, T) float in [-1, 1] -> (B, n_mel_channels, T // hop + 1) on the GPU.

        When gradients are enabled and ``y.requires_grad`` the result carries a ``grad_fn`` (the same launches, so the same
        bits): it keeps the spectrum and the mel rows (``kept_state_floats``) and ``backward()`` gives ``y`` a float32
        gradient of its shape.  ``precision`` ('fp32' or 'bf16x3') selects the two products of the backward only.  Two
        subgradients are definitions: the gradient passes where mel >= clip_val (torch's clamp rule), and a bin whose
        magnitude is exactly 0 gets gradient 0, where torch's sqrt gives NaN.  The range check costs a host
        synchronisation: training callers pass ``check_range=False``."""
        _precision(precision)
        if torch.is_grad_enabled() and torch.is_tensor(y) and y.requires_grad:
            return _MelSpectrogram.apply(self, y, check_range, precision)
        y = _device_signal(y, self.mel_basis)
        if check_range and not nv.validate_only():
            self._check_range(y)
        return self._mel_forward(y)[0]


class _MelSpectrogram(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stft, y, check_range, precision):
        ys = _device_signal(y, stft.mel_basis)
        if check_range and not nv.validate_only():
            stft._check_range(ys)
        out, spec, mel_rows = stft._mel_forward(ys)
        ctx.stft, ctx.kept, ctx.fast = stft, (spec, mel_rows), _PRECISIONS[precision]
        ctx.y_shape, ctx.y_device = tuple(ys.shape), y.device
        return out

    @staticmethod
    def backward(ctx, d_out):
        spec, mel_rows = _take_kept(ctx, "mel_spectrogram")
        d_out = d_out.to(device=spec.device, dtype=torch.float32).contiguous()
        d_y = ctx.stft._mel_backward(d_out, spec, mel_rows, ctx.y_shape[0], ctx.y_shape[1], ctx.fast)
        return None, d_y.to(ctx.y_device), None, None


class MelLoss(torch.nn.Module):
    """Masked mean absolute error between the log-mels of ``audio`` and ``target_mel``:

        loss = sum_{b, m, i < lengths_b} |mel_spectrogram(audio)[b, m, i] - target_mel[b, m, i]| / (n_mel sum_b lengths_b)

    ``MelLoss(stft)(audio, target_mel, lengths=None, precision='fp32')`` -> a scalar on the GPU.  ``audio`` is (B, T) or
    (B, 1, T) in [-1, 1] (not checked: the check would cost a host synchronisation per step), ``target_mel`` (B, n_mel, N)
    with N <= T // hop + 1, ``lengths`` the frames of every utterance (default N).  One autograd function from the samples to
    the scalar; it keeps the spectrum, the mel rows and the target.  ``precision`` as in ``mel_spectrogram``."""

    def __init__(self, stft):
        super().__init__()
        if not isinstance(stft, TacotronSTFT):
            raise TypeError("MelLoss needs a tacotron2_amd.audio.TacotronSTFT")
        self.stft = stft

    def forward(self, audio, target_mel, lengths=None, precision='fp32'):
        st = self.stft
        _precision(precision)
        audio = _squeeze_channel(audio)
        if audio.dim() != 2:
            raise ValueError("MelLoss: expected (B, T) or (B, 1, T) samples, got shape %s" % (tuple(audio.shape),))
        B, T = audio.shape
        if target_mel.dim() != 3 or target_mel.shape[0] != B or target_mel.shape[1] != st.n_mel_channels:
            raise ValueError("MelLoss: expected (%d, %d, N) target log-mels, got shape %s"
                             % (B, st.n_mel_channels, tuple(target_mel.shape)))
        n, N = T // st.stft_fn.hop_length + 1, target_mel.shape[2]
        if N < 1 or N > n:
            raise ValueError("MelLoss: the target has %d frames, %d samples give %d" % (N, T, n))
        lens = _lengths(lengths, B, N, "MelLoss: ")
        _require_device(st.mel_basis)
        return _MelLoss.apply(st, audio, target_mel, lens, precision)


class _MelLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stft, audio, target, lens, precision):
        y = _device_signal(audio, stft.mel_basis)
        dev = y.device
        out, spec, mel_rows = stft._mel_forward(y)
        B, n_mel, n = out.shape
        tgt = target.detach().to(device=dev, dtype=torch.float32).contiguous()
        lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev)
        count = n_mel * (sum(lens) if lens is not None else B * tgt.shape[2])
        slots = nv.mel_l1_slots(B, n_mel, n)
        partial = torch.empty(slots, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nv.mel_l1_fwd(out, tgt, lens_dev, count, partial)
        nv.wg_partial_sum(partial, slots, 1, loss)
        ctx.stft, ctx.kept, ctx.fast = stft, (spec, mel_rows, tgt, lens_dev), _PRECISIONS[precision]
        ctx.count, ctx.y_shape, ctx.y_device = count, tuple(y.shape), audio.device
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        spec, mel_rows, tgt, lens_dev = _take_kept(ctx, "MelLoss")
        stft, (B, T) = ctx.stft, ctx.y_shape
        dev = spec.device
        n = spec.shape[0] // B
        g = g.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        out = torch.empty(B, stft.n_mel_channels, n, dtype=torch.float32, device=dev)
        nv.mel_log_compress(mel_rows, out, stft.clip_val)            # the forward's bits again, rather than kept
        d_out = torch.empty_like(out)
        nv.mel_l1_bwd(out, tgt, lens_dev, g, ctx.count, d_out)
        d_y = stft._mel_backward(d_out, spec, mel_rows, B, T, ctx.fast)
        return None, d_y.to(ctx.y_device), None, None, None


class MultiResolutionSTFTLoss(torch.nn.Module):
    """The multi-resolution STFT loss of Parallel WaveGAN between ``audio`` (carries the gradient) and ``target_audio`` (never
    differentiated), DESIGN.md section 14.  A resolution r = (L, hop, win) is ``STFT(L, hop, win)``'s transform: reflect padding by
    L/2, n_r = T // hop + 1 frames, F_r = L/2 + 1 bins, unnormalised basis.  With m = sqrt(max(re^2 + im^2, eps)) of either signal
    and the sums over the whole batch, frames j < n_{r,b} = min(n_r, lengths_b // hop + 1) and all bins (C_r of them):

        sc_r = sqrt(sum (m_y - m_x)^2) / sqrt(sum m_y^2)            lm_r = sum |ln m_x - ln m_y| / C_r
        loss = (1/R) sum_r (sc_weight sc_r + mag_weight lm_r)

    ``forward(audio, target_audio, lengths=None, precision='fp32')`` -> a 0-d tensor on the GPU with a ``grad_fn`` to ``audio``.
    ``audio`` and ``target_audio`` are (B, T) or (B, 1, T) (no range check: it would cost a host synchronisation); of a longer
    target the first T samples are used.  ``lengths`` are samples per utterance (default T); the last counted frames of a shorter
    utterance straddle samples beyond ``lengths_b`` in both signals and still count, as in ``MelLoss``.  ``precision`` ('fp32' or
    'bf16x3') selects the products of the backward only.  One autograd function; it keeps the two spectra of every resolution, the
    frame counts and the coefficient buffer (``kept_state_floats``).  ``last_terms`` is the detached (R, 2) device tensor of
    (sc_r, lm_r) of the last forward.  Three subgradients are definitions: the clamp passes the gradient where re^2 + im^2 >= eps
    (torch's rule) and gives exactly 0 below, sign(0) = 0, and a resolution whose sum (m_y - m_x)^2 is 0 contributes gradient
    exactly 0 through sc_r (torch gives NaN).  sum m_y^2 == 0 is not guarded (it would give a non-finite loss); with eps > 0 a silent
    target has m_y = sqrt(eps) and cannot reach it.  There is no CPU path."""

    DEFAULT_RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
    MAX_RESOLUTIONS = 8

    def __init__(self, resolutions=None, window='hann', sc_weight=1.0, mag_weight=1.0, eps=1e-7):
        super().__init__()
        res = self.DEFAULT_RESOLUTIONS if resolutions is None else resolutions
        self.resolutions = self.check_resolutions(res)
        if not float(eps) > 0.0:
            raise ValueError("MultiResolutionSTFTLoss: eps must be positive, got %r" % (eps,))
        self.sc_weight, self.mag_weight, self.eps = float(sc_weight), float(mag_weight), float(eps)
        self.stfts = torch.nn.ModuleList([STFT(L, hop, win, window) for L, hop, win in self.resolutions])
        self.last_terms = None
        if torch.cuda.is_available():
            self.cuda()

    @classmethod
    def check_resolutions(cls, resolutions):
        """-> the resolutions as a tuple of (L, hop, win) int triples; ValueError with the offending values otherwise."""
        try:
            res = tuple(tuple(int(v) for v in r) for r in resolutions)
        except (TypeError, ValueError):
            raise ValueError("MultiResolutionSTFTLoss: resolutions must be (filter_length, hop_length, win_length) triples, got %r"
                             % (resolutions,))
        if not 1 <= len(res) <= cls.MAX_RESOLUTIONS:
            raise ValueError("MultiResolutionSTFTLoss: 1 to %d resolutions, got %d" % (cls.MAX_RESOLUTIONS, len(res)))
        for r in res:
            if len(r) != 3:
                raise ValueError("MultiResolutionSTFTLoss: a resolution is (filter_length, hop_length, win_length), got %r" % (r,))
            L, hop, win = r
            if L < 2 or L % 2 or hop < 1 or win < 1 or win > L or hop > L:
                raise ValueError("MultiResolutionSTFTLoss: resolution %r needs an even filter_length >= 2, 1 <= hop_length <= "
                                 "filter_length and 1 <= win_length <= filter_length" % (r,))
        return res

    def kept_state_floats(self, B, T):
        """Elements kept between the forward and the backward for (B, T) samples: both spectra (B n_r, 2 F_r) of every resolution,
        the (R, B) frame counts and the (R, 2) coefficients."""
        R = len(self.resolutions)
        return sum(2 * B * (T // hop + 1) * 2 * (L // 2 + 1) for L, hop, _ in self.resolutions) + R * B + 2 * R

    def forward(self, audio, target_audio, lengths=None, precision='fp32'):
        _precision(precision)
        audio, target_audio = _squeeze_channel(audio), _squeeze_channel(target_audio)
        if audio.dim() != 2:
            raise ValueError("MultiResolutionSTFTLoss: expected (B, T) or (B, 1, T) samples, got shape %s" % (tuple(audio.shape),))
        B, T = audio.shape
        if target_audio.dim() != 2 or target_audio.shape[0] != B or target_audio.shape[1] < T:
            raise ValueError("MultiResolutionSTFTLoss: expected a (%d, >= %d) target, got shape %s" % (B, T, tuple(target_audio.shape)))
        Lmax = max(L for L, _, _ in self.resolutions)
        if T <= Lmax // 2:
            raise ValueError("MultiResolutionSTFTLoss: signal of %d samples is too short to reflect-pad by %d" % (T, Lmax // 2))
        lens = _lengths(lengths, B, T, "MultiResolutionSTFTLoss: ", full=T)
        return _MultiResolutionSTFTLoss.apply(self, audio, target_audio, lens, precision)


class _MultiResolutionSTFTLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, audio, target, lens, precision):
        basis = mod.stfts[0].forward_basis
        x = _device_signal(audio, basis)
        dev, (B, T) = x.device, x.shape
        y = target.detach().to(device=dev, dtype=torch.float32)
        if y.stride(1) != 1:
            y = y.contiguous()
        y = y[:, :T]                                                   # a view: the pad reads the first T samples of every row
        R = len(mod.stfts)
        cnts = [[min(T // st.hop_length + 1, n // st.hop_length + 1) for n in lens] for st in mod.stfts]
        cnt_dev = torch.tensor(cnts, dtype=torch.int32).to(dev)
        specs, offs, counts = [], [0], []
        for r, st in enumerate(mod.stfts):
            F = st.cutoff
            spec, n = st.frame_spectra([x, y], st.forward_basis.view(2 * F, st.filter_length), 2 * F)   # rows of x, then rows of y
            specs.append(spec)
            offs.append(offs[-1] + nv.stft_loss_slots(B * n, F))
            counts.append(F * sum(cnts[r]))
        slots = torch.empty(3 * offs[-1], dtype=torch.float64, device=dev)
        for r, st in enumerate(mod.stfts):
            rows = specs[r].shape[0] // 2
            nv.stft_loss_fwd(specs[r][:rows], specs[r][rows:], cnt_dev[r], rows // B, st.cutoff, mod.eps,
                             slots[3 * offs[r]:3 * offs[r + 1]])
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        terms = torch.empty(R, 2, dtype=torch.float32, device=dev)
        coef = torch.empty(R, 2, dtype=torch.float32, device=dev)
        nv.stft_loss_finish(slots, offs, counts, mod.sc_weight, mod.mag_weight, loss, terms, coef)
        mod.last_terms = terms
        ctx.mod, ctx.kept, ctx.fast = mod, (specs, cnt_dev, coef), _PRECISIONS[precision]
        ctx.y_shape, ctx.y_device = (B, T), audio.device
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        specs, cnt_dev, coef = _take_kept(ctx, "MultiResolutionSTFTLoss")
        mod, (B, T) = ctx.mod, ctx.y_shape
        dev = coef.device
        f32 = dict(dtype=torch.float32, device=dev)
        g = g.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        R = len(mod.stfts)
        parts = torch.empty(R, B, T, **f32)
        for r, st in enumerate(mod.stfts):
            rows = specs[r].shape[0] // 2
            d_spec = torch.empty(rows, st.bwd_tables(dev)["Kp"], **f32)
            nv.stft_loss_bwd(specs[r][:rows], specs[r][rows:], cnt_dev[r], coef[r], g, rows // B, st.cutoff, mod.eps, d_spec)
            specs[r] = None
            st.spectrum_backward(d_spec, B, T, ctx.fast, out=parts[r])
        if R == 1:
            d_y = parts[0]
        else:
            d_y = torch.empty(B, T, **f32)
            nv.stft_loss_sum(parts, d_y)                               # r = 0 .. R - 1 in order, one writer per sample
        return None, d_y.to(ctx.y_device), None, None, None


def resample_geometry(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """-> (o, n, base, width) of DESIGN.md section 15: o = orig / gcd, n = new / gcd, base = min(o, n) rolloff, width =
    ceil(W o / base)."""
    import math
    orig_freq, new_freq, W = int(orig_freq), int(new_freq), int(lowpass_filter_width)
    if orig_freq < 1 or new_freq < 1:
        raise ValueError("resample: the rates must be positive, got %d -> %d" % (orig_freq, new_freq))
    if W < 1 or not 0.0 < float(rolloff) <= 1.0:
        raise ValueError("resample: lowpass_filter_width >= 1 and 0 < rolloff <= 1, got %r and %r" % (lowpass_filter_width, rolloff))
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    base = min(o, n) * float(rolloff)
    return o, n, base, int(math.ceil(W * o / base))


def resample_tables(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """The host tables of ``Resample`` (numpy), DESIGN.md section 15.  ``dense`` (n, 2 width + o) float32 is the definition:
    h[j][k] = sinc(t) cos^2(pi t / (2 W)) base / o with t = ((k - width) / o - j / n) base where |t| < W and exactly 0 elsewhere,
    computed in float64 and rounded once.  ``tab`` (n, S) and ``first`` (n) are its compact form: tab[j][s] = dense[j][first[j] +
    s], every tap with |t| < W inside.  ``btab`` (o, Sb), ``bfirst`` (o), ``wpad``, ``Kd`` are the same float32 coefficients
    regrouped for the adjoint: d_x[q o + r] = sum_s btab[r][s] d_y[q n + bfirst[r] + s - wpad], ascending output index."""
    o, n, base, width = resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
    W = int(lowpass_filter_width)
    K = 2 * width + o
    k = np.arange(K, dtype=np.float64)
    j = np.arange(n, dtype=np.float64)
    t = ((k[None, :] - width) / o - j[:, None] / n) * base
    inside = np.abs(t) < W
    pt = np.pi * t
    sinc = np.where(t == 0.0, 1.0, np.sin(pt) / np.where(t == 0.0, 1.0, pt))
    dense = np.where(inside, sinc * np.cos(pt / (2.0 * W)) ** 2 * (base / o), 0.0).astype(np.float32)

    def compact(values, mask):
        """Rows of `values` cut to the columns [first, first + S) that hold every True of `mask`."""
        cols = mask.shape[1]
        lo = mask.argmax(axis=1)
        hi = cols - mask[:, ::-1].argmax(axis=1)
        S = int((hi - lo).max())
        first = np.minimum(lo, cols - S).astype(np.int32)
        return np.ascontiguousarray(values[np.arange(mask.shape[0])[:, None], first[:, None] + np.arange(S)[None, :]]), first

    tab, first = compact(dense, inside)
    # the adjoint: input i = Q o + r is read by output m = (Q + c) n + j through tap k = r + width - c o
    cmin, cmax = -((width + o - 1) // o), (o - 1 + width) // o
    D = (cmax - cmin + 1) * n
    bdense = np.zeros((o, D), dtype=np.float32)
    bmask = np.zeros((o, D), dtype=bool)
    r = np.arange(o)
    for c in range(cmin, cmax + 1):
        kk = r + width - c * o
        ok = (kk >= 0) & (kk < K)
        cols = slice((c - cmin) * n, (c - cmin + 1) * n)
        bdense[ok, cols] = dense[:, kk[ok]].T
        bmask[ok, cols] = inside[:, kk[ok]].T
    btab, bfirst = compact(bdense, bmask)
    shift = int(bfirst.min())
    bfirst = (bfirst - shift).astype(np.int32)
    return {"o": o, "n": n, "width": width, "dense": dense, "tab": tab, "first": first, "btab": btab, "bfirst": bfirst,
            "wpad": -cmin * n - shift, "Kd": int(bfirst.max()) + btab.shape[1]}


class Resample(torch.nn.Module):
    """Sample-rate conversion on the GPU (csrc/resample.hip): band-limited sinc interpolation with a Hann
    window, ``resample_tables``' definition.  ``forward(x, lengths=None)`` takes (T,), (B, T) or (B, 1, T) float32 device samples
    and returns the same rank with ``output_length(T)`` = ceil(new T / orig) samples; with ``lengths`` (samples per utterance) the
    samples at and beyond them read as zero, the result is 0 beyond the new lengths, and (y, new lengths) is returned.  One
    autograd function, two launches in all; the only kept state is the lengths.  ``orig_freq == new_freq`` returns its input
    unchanged.  There is no CPU path."""

    def __init__(self, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
        super().__init__()
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.lowpass_filter_width, self.rolloff = int(lowpass_filter_width), float(rolloff)
        self.o, self.n, _, self.width = resample_geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
        self._host = None
        self._lazy = {}                 # per device: the four tables (plain attributes, not buffers)

    def host_tables(self):
        if self._host is None:
            self._host = resample_tables(self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff)
        return self._host

    def tables(self, device):
        """Device tables, built on first use: ``tab`` (n, S), ``first`` (n), ``btab`` (o, Sb), ``bfirst`` (o), with the host
        integers ``wpad`` and ``Kd`` of the adjoint."""
        def build(device):
            h = self.host_tables()
            out = dict((k, torch.from_numpy(h[k]).to(device)) for k in ("tab", "first", "btab", "bfirst"))
            out["wpad"], out["Kd"] = h["wpad"], h["Kd"]
            return out
        return _per_device(self._lazy, 'resample', device, build)

    def table_paths(self):
        """(forward, backward): 'lds' where the launch stages its phase table in LDS, 'memory' where it reads it from memory."""
        h = self.host_tables()
        fwd = nv.resample_plan(self.n, self.o, h["tab"].shape[1], 2 * self.width + self.o)[1]
        bwd = nv.resample_plan(self.o, self.n, h["btab"].shape[1], h["Kd"])[1]
        return tuple('lds' if p else 'memory' for p in (fwd, bwd))

    def output_length(self, T):
        """ceil(new T / orig) for an int or each element of a sequence."""
        if isinstance(T, (list, tuple)):
            return [self.output_length(v) for v in T]
        return -(-self.n * int(T) // self.o)

    def forward(self, x, lengths=None):
        if not torch.is_tensor(x) or x.dtype != torch.float32:
            raise TypeError("Resample: expected a float32 tensor, got %s" % (x.dtype if torch.is_tensor(x) else type(x).__name__))
        if x.dim() not in (1, 2, 3) or (x.dim() == 3 and x.shape[1] != 1) or x.shape[-1] < 1 or x.shape[0] < 1:
            raise ValueError("Resample: expected (T,), (B, T) or (B, 1, T) samples, got shape %s" % (tuple(x.shape),))
        _require_device(x)
        rows = x.reshape(-1, x.shape[-1])
        lens = _lengths(lengths, rows.shape[0], rows.shape[1], "Resample: ")
        if self.o == self.n:
            return x if lens is None else (x, list(lens))
        y = _Resample.apply(self, rows, lens)
        y = y.reshape(tuple(x.shape[:-1]) + (y.shape[-1],))
        return y if lens is None else (y, self.output_length(list(lens)))


class _Resample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, lens):
        xs = x.detach()
        if xs.stride(1) != 1:
            xs = xs.contiguous()
        tb = mod.tables(xs.device)
        B, T = xs.shape
        lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(xs.device)
        y = torch.empty(B, mod.output_length(T), dtype=torch.float32, device=xs.device)
        nv.resample_fwd(xs, lens_dev, y, tb["tab"], tb["first"], mod.o, mod.n, mod.width)
        ctx.mod, ctx.kept, ctx.x_shape = mod, (lens_dev,), (B, T)
        return y

    @staticmethod
    def backward(ctx, d_y):
        (lens_dev,) = _take_kept(ctx, "Resample")
        mod, (B, T) = ctx.mod, ctx.x_shape
        d_y = d_y.to(dtype=torch.float32)
        if d_y.stride(1) != 1:
            d_y = d_y.contiguous()
        tb = mod.tables(d_y.device)
        d_x = torch.empty(B, T, dtype=torch.float32, device=d_y.device)
        nv.resample_bwd(d_y, lens_dev, d_x, tb["btab"], tb["bfirst"], mod.o, mod.n, tb["wpad"], tb["Kd"])
        return None, d_x, None


_RESAMPLERS = {}


def resample(x, orig_freq, new_freq, lengths=None):
    """``Resample(orig_freq, new_freq)(x, lengths)`` with the modules (and so their tables) of the last few rate pairs cached."""
    key = (int(orig_freq), int(new_freq))
    mod = _RESAMPLERS.pop(key, None)
    if mod is None:
        mod = Resample(*key)
        while len(_RESAMPLERS) >= 8:
            _RESAMPLERS.pop(next(iter(_RESAMPLERS)))
    _RESAMPLERS[key] = mod              # most recently used last
    return mod(x, lengths)


_resample = resample                    # for the callers below whose flag is named ``resample``


DTW_MAX_FRAMES = 4096
DTW_MAX_COEF = 32
MCD_DB = 10.0 / np.log(10.0) * np.sqrt(2.0)


def cepstral_basis(n_mel, n_coef=13):
    """(n_coef, n_mel) float32: row k-1 is sqrt(2 / N) cos(pi k (m + 1/2) / N), k = 1 ... n_coef, the orthonormal DCT-II without
    c0, computed in float64 and rounded once."""
    n_mel, n_coef = int(n_mel), int(n_coef)
    if not 1 <= n_coef <= DTW_MAX_COEF:
        raise ValueError("n_coef must lie in [1, %d], got %d" % (DTW_MAX_COEF, n_coef))
    if n_mel < 1:
        raise ValueError("n_mel must be positive, got %d" % n_mel)
    k = np.arange(1, n_coef + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mel, dtype=np.float64)[None, :]
    return (np.sqrt(2.0 / n_mel) * np.cos(np.pi * k * (m + 0.5) / n_mel)).astype(np.float32)


_CEPSTRAL_BASES = {}


def _frames(t, who, what):
    """A float32 rank-3 device tensor, or an error in the words of the neighbouring modules."""
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError("%s: expected a float32 tensor, got %s" % (who, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if t.dim() != 3 or min(t.shape) < 1:
        raise ValueError("%s: expected %s, got shape %s" % (who, what, tuple(t.shape)))
    _require_device(t)
    return t.detach()


def mel_cepstrum(mel, lengths=None, n_coef=13):
    """(B, n_mel, T) natural-log mel (what ``TacotronSTFT.mel_spectrogram`` returns) -> (B, T, n_coef) float32 mel cepstra
    c_k = sqrt(2 / N) sum_m x_m cos(pi k (m + 1/2) / N), k = 1 ... n_coef, summed in ascending m (csrc/dtw.hip).  Rows at and
    beyond ``lengths`` are zeros.  No gradient; there is no CPU path."""
    mel = _frames(mel, "mel_cepstrum", "(B, n_mel, T) log-mels")
    B, N, T = mel.shape
    key = (N, int(n_coef))
    if key not in _CEPSTRAL_BASES:
        _CEPSTRAL_BASES[key] = {"host": torch.from_numpy(cepstral_basis(N, n_coef))}
    if N * key[1] > 8192:
        raise ValueError("mel_cepstrum: n_coef x n_mel must not exceed 8192, got %d x %d" % (key[1], N))
    basis = _per_device(_CEPSTRAL_BASES[key], 'basis', mel.device, lambda d: _CEPSTRAL_BASES[key]["host"].to(d))
    lens = None if lengths is None else _lengths(lengths, B, T, "mel_cepstrum: ")
    if mel.stride(2) != 1 and T > 1:
        mel = mel.contiguous()
    out = torch.empty(B, T, key[1], dtype=torch.float32, device=mel.device)
    nv.mel_cepstrum(mel, None if lens is None else torch.tensor(lens, dtype=torch.int32).to(mel.device), basis, out)
    return out


def dtw(x, y, x_lengths=None, y_lengths=None, return_path=False):
    """Dynamic time warping of x (B, Tx, K) against y (B, Ty, K), float32 on the device (csrc/dtw.hip):
    Euclidean local cost, steps (1,1), (1,0), (0,1), ties taken in that order.  -> ``cost`` (B,) float32, the accumulated cost of
    the optimal path, ``steps`` (B,) int32, its number of cells, and with ``return_path`` also ``path`` (B, max n_x + max n_y - 1,
    2) int32: the cells (i, j) from (0, 0) to (n_x - 1, n_y - 1), -1 beyond ``steps``.  Lengths lie in [1, min(T, 4096)]."""
    x = _frames(x, "dtw", "(B, T, K) frames")
    y = _frames(y, "dtw", "(B, T, K) frames")
    if x.device != y.device:
        raise ValueError("dtw: the two sequences live on %s and %s" % (x.device, y.device))
    if x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2]:
        raise ValueError("dtw: expected (B, Tx, K) and (B, Ty, K), got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    B, Tx, K = x.shape
    Ty = y.shape[1]
    if not 1 <= K <= DTW_MAX_COEF:
        raise ValueError("dtw: K must lie in [1, %d], got %d" % (DTW_MAX_COEF, K))
    lx = _lengths(x_lengths, B, min(Tx, DTW_MAX_FRAMES), "dtw: x_", full=Tx)
    ly = _lengths(y_lengths, B, min(Ty, DTW_MAX_FRAMES), "dtw: y_", full=Ty)
    dev = x.device
    na, nb = (torch.tensor(v, dtype=torch.int32).to(dev) for v in (lx, ly))
    cost = torch.empty(B, dtype=torch.float32, device=dev)
    steps = torch.empty(B, dtype=torch.int32, device=dev)
    x, y = x.contiguous(), y.contiguous()
    if not return_path:
        nv.dtw(x, y, na, nb, cost, steps)
        return cost, steps
    slab = torch.empty(B, max(lx), max(ly), dtype=torch.uint8, device=dev)
    path = torch.empty(B, max(lx) + max(ly) - 1, 2, dtype=torch.int32, device=dev)
    nv.dtw(x, y, na, nb, cost, steps, slab)
    nv.dtw_backtrack(slab, na, nb, steps, Tx, Ty, path)
    return cost, steps, path


class MelCepstralDistortion(torch.nn.Module):
    """Mel-cepstral distortion under dynamic time warping, in dB per pair.  ``forward(mel_a, mel_b,
    len_a=None, len_b=None)`` takes two (B, n_mel, T) natural-log mels of any two lengths and returns (B,) float32:
    (10 / ln 10) sqrt(2) cost / steps with ``cost`` and ``steps`` those of ``dtw`` over the ``mel_cepstrum`` of each side.
    ``last`` holds the ``cost``, ``steps``, ``len_a`` and ``len_b`` of the latest call (and ``path`` when ``return_path``).  An
    evaluation figure: it runs under ``no_grad`` and returns tensors without a ``grad_fn``.  There is no CPU path."""

    def __init__(self, n_coef=13, return_path=False):
        super().__init__()
        if not 1 <= int(n_coef) <= DTW_MAX_COEF:
            raise ValueError("n_coef must lie in [1, %d], got %d" % (DTW_MAX_COEF, int(n_coef)))
        self.n_coef, self.return_path = int(n_coef), bool(return_path)
        self.last = None

    @torch.no_grad()
    def forward(self, mel_a, mel_b, len_a=None, len_b=None):
        mel_a = _frames(mel_a, "MelCepstralDistortion", "(B, n_mel, T) log-mels")
        mel_b = _frames(mel_b, "MelCepstralDistortion", "(B, n_mel, T) log-mels")
        if mel_a.shape[:2] != mel_b.shape[:2]:
            raise ValueError("MelCepstralDistortion: expected two (B, n_mel, T) log-mels of one B and n_mel, got %s and %s"
                             % (tuple(mel_a.shape), tuple(mel_b.shape)))
        B = mel_a.shape[0]
        la = _lengths(len_a, B, min(mel_a.shape[2], DTW_MAX_FRAMES), "MelCepstralDistortion: len_a: ", full=mel_a.shape[2])
        lb = _lengths(len_b, B, min(mel_b.shape[2], DTW_MAX_FRAMES), "MelCepstralDistortion: len_b: ", full=mel_b.shape[2])
        ca = mel_cepstrum(mel_a[:, :, :max(la)], la, self.n_coef)
        cb = mel_cepstrum(mel_b[:, :, :max(lb)], lb, self.n_coef)
        out = dtw(ca, cb, la, lb, return_path=self.return_path)
        cost, steps = out[0], out[1]
        self.last = {"cost": cost, "steps": steps, "len_a": la, "len_b": lb}
        if self.return_path:
            self.last["path"] = out[2]
        return cost * (float(MCD_DB) / steps.to(torch.float32))


def yin(y, lengths=None, sr=22050, frame_length=1024, hop_length=256, fmin=60.0, fmax=800.0, threshold=0.1, return_dprime=False):
    """F0 by YIN (csrc/yin.hip) of y (B, T) or (T,), float32 on the device, unit stride along time.
    Utterance b has ``lengths[b] // hop_length + 1`` frames, the mel front end's count; frame t is centred on sample t hop_length
    and padded with zeros.  -> ``f0`` (B, frames) float32 in Hz (the best estimate on unvoiced frames too), ``voiced`` (B, frames)
    bool, ``aperiodicity`` (B, frames) float32 = d'(tau); with ``return_dprime`` also the slab (B, frames, tau_max + 2) of
    d'(0 .. tau_max + 1).  Frames at and beyond an utterance's count are 0 / False / 0.  Not differentiable: an estimator with a
    discrete choice of lag; it detaches its input and returns tensors without a ``grad_fn``.  There is no CPU path."""
    if not torch.is_tensor(y) or y.dtype != torch.float32:
        raise TypeError("yin: expected a float32 tensor, got %s" % (y.dtype if torch.is_tensor(y) else type(y).__name__))
    if y.dim() == 1:
        y = y.unsqueeze(0)
    if y.dim() != 2 or min(y.shape) < 1:
        raise ValueError("yin: expected (B, T) or (T,) samples, got shape %s" % (tuple(y.shape),))
    if y.shape[1] > 1 and y.stride(1) != 1:
        raise ValueError("yin: the signal must have unit stride along time, got stride %s" % (y.stride(),))
    _require_device(y)
    y = y.detach()
    B, T = y.shape
    tau_min, tau_max = nv.yin_plan(sr, frame_length, hop_length, fmin, fmax)
    lens = _lengths(lengths, B, T, "yin: ")
    dev = y.device
    frames = T // int(hop_length) + 1
    f0 = torch.empty(B, frames, dtype=torch.float32, device=dev)
    ap = torch.empty(B, frames, dtype=torch.float32, device=dev)
    voiced = torch.empty(B, frames, dtype=torch.uint8, device=dev)
    slab = torch.empty(B, frames, tau_max + 2, dtype=torch.float32, device=dev) if return_dprime else None
    nv.yin(y, None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev), frame_length, hop_length, tau_min, tau_max,
           sr, threshold, f0, voiced, ap, slab)
    out = (f0, voiced.view(torch.bool), ap)
    return out + (slab,) if return_dprime else out


def f0_metrics(f0_a, voiced_a, f0_b, voiced_b, len_a=None, len_b=None, path=None, steps=None):
    """The pitch figures of B pairs of F0 tracks (B, Ta) and (B, Tb), over the frames ``path`` pairs: the (B, L, 2) int32 path of
    ``dtw`` / ``MelCepstralDistortion(return_path=True)`` with its ``steps`` (entries beyond ``steps`` or below 0 are left out).
    Without a path, frame i is paired with frame i up to the shorter of ``len_a`` and ``len_b`` (None: all frames).  -> a dict of
    (B,) tensors: ``f0_rmse_cents`` (root mean square of 1200 log2(fa / fb) over the steps where both are voiced), ``f0_corr``
    (Pearson correlation over the same steps), ``vuv_error`` (share of steps whose flags differ), ``gross_pitch_error`` (share of
    both-voiced steps with |fa / fb - 1| > 0.2), all float64, and ``voiced_steps`` (int64).  A pair with no both-voiced step gets
    NaN for the first two and for ``gross_pitch_error``; so does the correlation of a constant track.  Plain torch in float64."""
    if f0_a.dim() != 2 or f0_b.dim() != 2 or f0_a.shape != voiced_a.shape or f0_b.shape != voiced_b.shape \
            or f0_a.shape[0] != f0_b.shape[0]:
        raise ValueError("f0_metrics: expected (B, Ta) and (B, Tb) tracks with flags of their shapes, got %s %s %s %s"
                         % (tuple(f0_a.shape), tuple(voiced_a.shape), tuple(f0_b.shape), tuple(voiced_b.shape)))
    B, Ta = f0_a.shape
    Tb = f0_b.shape[1]
    dev = f0_a.device
    la = torch.tensor(_lengths(len_a, B, Ta, "f0_metrics: len_a: ", full=Ta), device=dev)
    lb = torch.tensor(_lengths(len_b, B, Tb, "f0_metrics: len_b: ", full=Tb), device=dev)
    if path is None:
        n = torch.minimum(la, lb)
        idx = torch.arange(int(n.max()), device=dev)[None, :].expand(B, -1)
        ia, ib, valid = idx, idx, idx < n[:, None]
    else:
        if path.dim() != 3 or path.shape[0] != B or path.shape[2] != 2:
            raise ValueError("f0_metrics: expected a (B, L, 2) path, got %s" % (tuple(path.shape),))
        ia, ib = path[..., 0].long(), path[..., 1].long()
        valid = (ia >= 0) & (ib >= 0) & (ia < la[:, None]) & (ib < lb[:, None])
        if steps is not None:
            valid &= torch.arange(path.shape[1], device=dev)[None, :] < torch.as_tensor(steps, device=dev).long()[:, None]
    ia, ib = ia.clamp(0, Ta - 1), ib.clamp(0, Tb - 1)
    fa, fb = f0_a.double().gather(1, ia), f0_b.double().gather(1, ib)
    va, vb = voiced_a.bool().gather(1, ia) & valid, voiced_b.bool().gather(1, ib) & valid
    both = va & vb
    nb = both.sum(1)
    nan = torch.full((B,), float('nan'), dtype=torch.float64, device=dev)
    one = torch.ones((), dtype=torch.float64, device=dev)
    ra, rb = torch.where(both, fa, one), torch.where(both, fb, one)
    cents = 1200.0 * torch.log2(ra / rb)
    cnt = nb.clamp(min=1).double()
    rmse = torch.sqrt((cents * cents).sum(1) / cnt)
    gross = (both & ((ra / rb - 1.0).abs() > 0.2)).sum(1).double() / cnt
    w = both.double()
    ca, cb = (fa - ((fa * w).sum(1) / cnt)[:, None]) * w, (fb - ((fb * w).sum(1) / cnt)[:, None]) * w
    corr = (ca * cb).sum(1) / torch.sqrt((ca * ca).sum(1) * (cb * cb).sum(1))          # 0 / 0 = NaN for a constant track
    some = nb > 0
    return {"f0_rmse_cents": torch.where(some, rmse, nan), "f0_corr": torch.where(some, corr, nan),
            "vuv_error": ((va != vb) & valid).sum(1).double() / valid.sum(1).clamp(min=1).double(),
            "gross_pitch_error": torch.where(some, gross, nan), "voiced_steps": nb}


def precompute_mels(filelist, hparams, out_dir, out_filelist=None, resample=False):
    """Run every wav of a ``path|text`` filelist through the GPU front end once and write
    ``<out_dir>/<stem>.npy`` (n_mel, frames) float32 — the files the reference's
    ``load_mel_from_disk=True`` path reads (hparams.py:27, data_utils.py:50-55).  Optionally writes
    the matching filelist.  Returns the number of utterances.  ``resample=True`` converts a file at another
    rate to ``hparams.sampling_rate`` on the GPU (``Resample``) instead of refusing it."""
    from .utils import load_filepaths_and_text, load_wav_to_torch
    stft = TacotronSTFT(hparams.filter_length, hparams.hop_length, hparams.win_length, hparams.n_mel_channels,
                        hparams.sampling_rate, hparams.mel_fmin, hparams.mel_fmax)
    os.makedirs(out_dir, exist_ok=True)
    rows = load_filepaths_and_text(filelist)
    lines = []
    for fields in rows:
        audio, sr = load_wav_to_torch(fields[0])
        audio = (audio / hparams.max_wav_value).unsqueeze(0)
        if sr != hparams.sampling_rate:
            if not resample:
                raise ValueError("%s: sampling rate %d, expected %d" % (fields[0], sr, hparams.sampling_rate))
            audio = _resample(audio.to(stft.mel_basis.device), sr, hparams.sampling_rate).clamp_(-1.0, 1.0)
        mel = stft.mel_spectrogram(audio).squeeze(0)
        dst = os.path.join(out_dir, os.path.splitext(os.path.basename(fields[0]))[0] + '.npy')
        np.save(dst, mel.cpu().numpy())
        lines.append('|'.join([dst] + fields[1:]))
    if out_filelist:
        with open(out_filelist, 'w', encoding='utf-8') as fh:
            fh.write('\n'.join(lines) + '\n')
    return len(rows)
