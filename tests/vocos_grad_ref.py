"""The differentiable composition of tests/vocos_ref.py (``VocosRef.forward`` runs under no_grad) and float64 torch models
of the formulas of the row kernels of csrc/vocos_bwd.hip.  The gradient reference of tests/test_vocos_grad_cpu.py and
tests/test_zz17_vocos_grad_gpu.py is torch autograd over ``audio`` with the linear loss L = sum(audio * r): the tests see the
Jacobian transpose and nothing else."""
import math

import torch
import torch.nn.functional as F

import vocos_ref as vr

# (geometry, frames per utterance, mel seed) of every gradient case the GPU tests run; weights are make_ref(name, WEIGHT_SEED).
# A log-magnitude on the other side of log(100) than in float64 is a discontinuity of the model, not an error of a kernel: one
# such bin moves the mels' and most parameters' gradients by 1e-1 (tests/test_vocos_grad_cpu.py shows it in float64).  So the
# seeds keep every float64 log-magnitude clear of the clamp, and the CPU suite asserts it: by CLAMP_MARGIN everywhere, which
# covers float32 and split-bf16, and on the small geometries by BF16_CLAMP_MARGIN, since with the blocks' products in bf16
# the log-magnitudes are off by a few 1e-3 (bins 2.3e-3 and 2.7e-3 from the clamp were seen to change sides on the MI355X,
# none further away).  V has 32,832 bins at B = 1 x 64 with 1 % of them above the clamp: the nearest lies 8.7e-4 away on
# average and no seed gives 1e-2; seed 2 gives 3.0e-3.  The GPU test asserts for every case and precision that the forward it
# differentiates has every bin on the float64 side.
WEIGHT_SEED = 0
GPU_CASES = [('small', [40, 40], 18), ('odd', [40, 40], 22), ('center', [40, 40], 18), ('V', [64], 2), ('small', [3, 1, 140], 51)]
CLAMP_MARGIN = 1e-3
BF16_CLAMP_MARGIN = 1e-2


def clamp_margin(name):
    return CLAMP_MARGIN if name == 'V' else BF16_CLAMP_MARGIN

def audio(ref, mel, lengths=None, flips=()):
    """``VocosRef.forward`` under autograd; with ``lengths`` every utterance alone, zero beyond its samples.  ``flips``:
    (utterance, bin, frame) whose side of the clamp is inverted (a model of a bin that a lower precision puts there)."""
    c = ref.config
    if lengths is not None:
        hop = c['hop_length']
        T = hop * mel.shape[2] if c['padding'] == 'same' else hop * (mel.shape[2] - 1)
        out = []
        for b, n in enumerate(lengths):
            a = audio(ref, mel[b:b + 1, :, :n], flips=[(0, k, j) for bb, k, j in flips if bb == b])
            out.append(F.pad(a, (0, T - a.shape[2])))
        return torch.cat(out, 0)
    m, p = ref.head(ref.backbone(mel))
    mag = torch.clamp(torch.exp(m), max=vr.CLAMP)
    if flips:
        over = torch.exp(m.detach()) > vr.CLAMP
        for b, k, j in flips:
            over[b, k, j] = ~over[b, k, j]
        mag = torch.where(over, torch.full_like(m, vr.CLAMP), torch.exp(m))
    S = torch.complex(mag * torch.cos(p), mag * torch.sin(p))
    return vr.istft(S, ref.w['head.istft.window'], c['hop_length'], c['padding'])[:, None, :]


def log_magnitudes(ref, mel, lengths=None):
    with torch.no_grad():
        if lengths is None:
            return ref.head(ref.backbone(mel))[0].flatten()
        return torch.cat([ref.head(ref.backbone(mel[b:b + 1, :, :n]))[0].flatten() for b, n in enumerate(lengths)])


def loss_weights(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) / math.sqrt(shape[-1])


def grads(ref, mel, r, lengths=None, flips=()):
    """{parameter name: gradient, 'mel': gradient} of sum(audio * r) in the dtype of ``ref`` and ``mel``."""
    names = [n for n, _, _ in vr.shapes(ref.config)]
    leaves = {n: ref.w[n].detach().clone().requires_grad_(True) for n in names}
    leaves['head.istft.window'] = ref.w['head.istft.window']
    x = mel.detach().clone().requires_grad_(True)
    a = audio(vr.VocosRef(ref.config, leaves), x, lengths, flips)
    (a * r.to(a.dtype)).sum().backward()
    out = {n: leaves[n].grad for n in names}
    out['mel'] = x.grad
    return out


# ---- models of the kernels' formulas, on packed row images ----------------------------------------------------------------
def ola_bwd(d_audio, wsq, lens, offs, P, hop, trim):
    """d_frames [P][L]: frame row j of utterance b, sample t reads d_audio[b][j hop + t - trim] / env, inside the utterance."""
    L = wsq.numel()
    out = torch.zeros(P, L, dtype=d_audio.dtype)
    T = d_audio.shape[2]
    for b, (o, n) in enumerate(zip(offs, lens)):
        env = vr.overlap_add((wsq.to(d_audio.dtype))[None, :, None].expand(1, L, n), hop)[0]
        Tb = min(T, hop * (n - 1) + L - 2 * trim)
        for j in range(n):
            for t in range(L):
                ts = j * hop + t - trim
                if 0 <= ts < Tb:
                    out[o + j, t] = d_audio[b, 0, ts] / env[j * hop + t]
    return out


def polar_bwd(Y, dS, Fb, clamp=vr.CLAMP):
    """[d_m | d_p] from Y = [m | p] and interleaved dS."""
    m, p = Y[:, :Fb], Y[:, Fb:2 * Fb]
    dre, dim = dS[:, 0:2 * Fb:2], dS[:, 1:2 * Fb:2]
    e = torch.exp(m)
    mag = torch.clamp(e, max=clamp)
    dm = torch.where(e <= clamp, mag * (torch.cos(p) * dre + torch.sin(p) * dim), torch.zeros_like(e))
    dp = mag * (torch.cos(p) * dim - torch.sin(p) * dre)
    return torch.cat([dm, dp], 1)


def gelu_bwd(u, dh):
    return dh * (0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi))


def gamma_bwd(dx, y2, gamma):
    """(d_y2, d_gamma)."""
    return gamma * dx, (dx * y2).sum(0)


def dwconv(X, w, cb, real):
    """The forward on a packed image with zero halos: w [taps][D]."""
    taps = w.shape[0]
    half = (taps - 1) // 2
    Xp = F.pad(X, (0, 0, half, half))
    y = cb + sum(Xp[t:t + X.shape[0]] * w[t] for t in range(taps))
    return y * real[:, None]


def ln_bwd(y, lw, g, real, eps=vr.LN_EPS):
    """(d_z, d_lw, d_lb) of out = xh lw + lb over the real rows of y, g = d_out."""
    D = y.shape[1]
    mean = y.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((y - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (y - mean) * rstd
    wd = lw * g
    dz = rstd * (wd - wd.mean(1, keepdim=True) - xh * (wd * xh).mean(1, keepdim=True))
    r = real[:, None].to(y.dtype)
    return dz * r, (g * xh * r).sum(0), (g * r).sum(0)


def dw_bwd(dz, X, w, res, real):
    """(d_x, d_w [taps][D], d_bias) over the finished d_z image (zero halos)."""
    taps = w.shape[0]
    half = (taps - 1) // 2
    P = X.shape[0]
    Zp, Xp = F.pad(dz, (0, 0, half, half)), F.pad(X, (0, 0, half, half))
    dx = res + sum(w[t] * Zp[2 * half - t:2 * half - t + P] for t in range(taps))
    dw = torch.stack([(dz * Xp[t:t + P]).sum(0) for t in range(taps)])
    return dx * real[:, None], dw, dz.sum(0)
