"""The differentiable restatement of the mel front end (oracle/audio_oracle.py's arithmetic: reflect ``F.pad``, ``conv1d`` with
the windowed basis at stride hop, ``librosa_mel``, log of clamp) in any dtype, float64 by default, and numpy / torch models of
the row kernels of csrc/audio_bwd.hip.  Two things differ from the oracle: the magnitude is ``where(p > 0, sqrt(p), 0)``, so
that a bin of magnitude exactly 0 has gradient 0 (the product's definition; torch's sqrt gives NaN there), and torch autograd
differentiates it.  The gradient reference of tests/test_audio_grad_cpu.py and tests/test_zz18_audio_grad_gpu.py."""
import functools
import math

import torch
import torch.nn.functional as F

from oracle import audio_oracle as ao

CLIP = 1e-5
DEFAULT = dict(filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, sampling_rate=22050, mel_fmin=0.0,
               mel_fmax=8000.0)
SMALL = dict(filter_length=512, hop_length=128, win_length=400, n_mel_channels=40, sampling_rate=16000, mel_fmin=50.0,
             mel_fmax=7600.0)
# name -> (geometry, B, T): A the shortest legal signal (both mirrors fold onto the same samples), B odd and no multiple of hop,
# C win_length < filter_length and three utterances
CASES = {'A': (DEFAULT, 1, 513), 'B': (DEFAULT, 1, 2125), 'C': (SMALL, 3, 1500)}
SIGNAL_SEED = 7
MIN_MEL = 1e-3                    # every float64 mel bin of the cases is at least this (100 x the clamp)
MIN_DIFF = 0.1                    # every |log-mel - target| of the L1 cases is at least this: no precision can flip a sign


def signal(name):
    """(B, T) float64: clamp(0.1 randn, -1, 1) from manual_seed(7)."""
    _, B, T = CASES[name]
    g = torch.Generator().manual_seed(SIGNAL_SEED)
    return torch.clamp(0.1 * torch.randn(B, T, generator=g, dtype=torch.float64), -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def _tables(key):
    geom = dict(key)
    fb = ao.forward_basis(geom['filter_length'], geom['win_length'])
    mb = torch.from_numpy(ao.librosa_mel(geom['sampling_rate'], geom['filter_length'], geom['n_mel_channels'],
                                         geom['mel_fmin'], geom['mel_fmax'])).float()
    return fb, mb


def tables(geom, dtype=torch.float64, device='cpu'):
    """(forward basis (2F, 1, L), mel basis (n_mel, F)): the oracle's float32 tables in ``dtype``."""
    fb, mb = _tables(tuple(sorted(geom.items())))
    return fb.to(device=device, dtype=dtype), mb.to(device=device, dtype=dtype)


def mel(y, geom):
    """(B, n_mel, n) linear mels of y (B, T) in y's dtype, differentiable."""
    L, hop = geom['filter_length'], geom['hop_length']
    fb, mb = tables(geom, y.dtype, y.device)
    B, T = y.shape
    x = F.pad(y.view(B, 1, 1, T), (L // 2, L // 2, 0, 0), mode='reflect').squeeze(1)
    ft = F.conv1d(x, fb, stride=hop, padding=0)
    cutoff = L // 2 + 1
    re, im = ft[:, :cutoff, :], ft[:, cutoff:, :]
    p = re ** 2 + im ** 2
    pos = p > 0
    mag = torch.where(pos, torch.sqrt(torch.where(pos, p, torch.ones_like(p))), torch.zeros_like(p))
    return torch.matmul(mb, mag)


def logmel(y, geom):
    return torch.log(torch.clamp(mel(y, geom), min=CLIP))


def loss_weights(shape, seed):
    """The smooth loss of the parity tests: sum(out * r), r a seeded randn / sqrt(numel)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) / math.sqrt(math.prod(shape))


def l1_target(lm64, seed):
    """logmel64 + s u, u uniform in [0.1, 0.5], s a seeded random sign: no difference is closer to zero than 0.1."""
    g = torch.Generator().manual_seed(seed)
    u = 0.1 + 0.4 * torch.rand(lm64.shape, generator=g, dtype=torch.float64)
    s = torch.where(torch.rand(lm64.shape, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    return lm64.detach() + s * u


def l1_loss(out, target, lengths=None):
    """sum_{b, m, i < lengths_b} |out - target| / (n_mel sum lengths_b); target (B, n_mel, N), N <= out's frames."""
    B, n_mel, N = target.shape
    lens = [N] * B if lengths is None else list(lengths)
    mask = (torch.arange(N, device=out.device)[None, :] < torch.tensor(lens, device=out.device)[:, None])[:, None, :]
    d = (out[:, :, :N] - target.to(out.dtype)).abs() * mask.to(out.dtype)
    return d.sum() / (n_mel * sum(lens))


def grad_smooth(y, geom, r):
    """d/dy of sum(logmel(y) * r) in y's dtype."""
    x = y.detach().clone().requires_grad_(True)
    (logmel(x, geom) * r.to(x.dtype)).sum().backward()
    return x.grad


def loss_and_grad_l1(y, geom, target, lengths=None):
    x = y.detach().clone().requires_grad_(True)
    loss = l1_loss(logmel(x, geom), target, lengths)
    loss.backward()
    return loss.detach(), x.grad


# ---- models of the kernels' formulas -------------------------------------------------------------------------------------
def log_bwd(d_out, mel_rows, clip=CLIP):
    """d_mel (B n, n_mel) from d_out (B, n_mel, n) and the mel rows."""
    B, n_mel, n = d_out.shape
    g = d_out.permute(0, 2, 1).reshape(B * n, n_mel)
    return torch.where(mel_rows >= clip, g / mel_rows, torch.zeros_like(g))


def magnitude_bwd(d_mag, spec, Fb, Kp):
    """d_spec (R, Kp) = [d_re | d_im | 0] from spec (R, 2F) = [re | im]; the kernel's operations in its order."""
    re, im = spec[:, :Fb], spec[:, Fb:2 * Fb]
    mag = torch.sqrt(re * re + im * im)
    ok = mag != 0
    g = torch.where(ok, d_mag[:, :Fb] / torch.where(ok, mag, torch.ones_like(mag)), torch.zeros_like(mag))
    out = torch.zeros(spec.shape[0], Kp, dtype=spec.dtype)
    out[:, :Fb], out[:, Fb:2 * Fb] = g * re, g * im
    return out


def frames_fold(d_frames, B, T, L, hop):
    """d_y (B, T): overlap-add of the frame gradients into the padded signal, then the transpose of the reflect pad (index_add
    over the padded positions through torch's own reflect indices)."""
    n, pad = T // hop + 1, L // 2
    idx = F.pad(torch.arange(T, dtype=torch.float64).view(1, 1, 1, T), (pad, pad, 0, 0), mode='reflect').view(-1).long()
    out = torch.zeros(B, T, dtype=d_frames.dtype)
    for b in range(B):
        padded = torch.zeros(T + 2 * pad, dtype=d_frames.dtype)
        for j in range(n):
            padded[j * hop:j * hop + L] += d_frames[b * n + j]
        out[b].index_add_(0, idx, padded)
    return out


def l1_bwd(out, target, lens, g, count):
    B, n_mel, n = out.shape
    N = target.shape[2]
    d = torch.zeros_like(out)
    for b in range(B):
        k = N if lens is None else int(lens[b])
        d[b, :, :k] = torch.sign(out[b, :, :k] - target[b, :, :k]) * (g / count)
    return d
