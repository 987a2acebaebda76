"""The float64 restatement of the sample-rate converter in plain torch, for the tests only: the dense
(n, 2 width + o) table with exact zeros outside |t| < W, zero padding, one strided ``conv1d``, truncation to ceil(n T / o), input
zeroing by ``lengths``; differentiable by torch autograd in any float dtype.  ``dense_table(..., zero_outside=False)`` is the
unclamped-zero dense formulation the definition departs from: t clamped to +-W, cos^2(pi / 2) left in the outer taps."""
import math

import torch


def geometry(orig, new, W=6, rolloff=0.99):
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * rolloff
    return o, n, base, int(math.ceil(W * o / base))


def dense_table(orig, new, W=6, rolloff=0.99, zero_outside=True, dtype=torch.float64):
    """(n, 2 width + o) in float64 (rounded to `dtype` at the end)."""
    o, n, base, width = geometry(orig, new, W, rolloff)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, :] / o
    t = (torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx) * base
    inside = t.abs() < W
    t = t.clamp(-W, W)
    window = torch.cos(t * math.pi / W / 2) ** 2
    t = t * math.pi
    h = torch.where(t == 0, torch.ones_like(t), t.sin() / torch.where(t == 0, torch.ones_like(t), t)) * window * (base / o)
    if zero_outside:
        h = torch.where(inside, h, torch.zeros_like(h))
    return h.to(dtype)


def output_length(orig, new, T):
    o, n, _, _ = geometry(orig, new)
    return -(-n * int(T) // o)


def resample(x, orig, new, lengths=None, W=6, rolloff=0.99, table=None, conv=True):
    """x (B, T) of any float dtype -> (B, ceil(n T / o)) in that dtype, the table rounded once to it; samples at and beyond
    ``lengths`` read as zero and the result is exactly 0 at and beyond the new lengths.  ``conv=False`` states the strided
    ``conv1d`` as what it is, the windows of the padded signal at stride o times the table (``unfold`` and ``matmul``): the same
    sums, and on a GPU no convolution kernel is compiled per shape, which is what keeps the GPU tests quick."""
    o, n, _, width = geometry(orig, new, W, rolloff)
    B, T = x.shape
    h = (dense_table(orig, new, W, rolloff) if table is None else table).to(device=x.device, dtype=x.dtype)
    if lengths is not None:
        keep = torch.arange(T, device=x.device)[None, :] < torch.tensor(list(lengths), device=x.device)[:, None]
        x = torch.where(keep, x, torch.zeros_like(x))
    xp = torch.nn.functional.pad(x, (width, width + o))
    if conv:
        y = torch.nn.functional.conv1d(xp[:, None, :], h[:, None, :], stride=o).transpose(1, 2)      # (B, Q, n)
    else:
        y = torch.matmul(xp.unfold(-1, h.shape[1], o), h.t())
    y = y.reshape(B, -1)[:, :output_length(orig, new, T)]
    if lengths is not None:
        new_len = torch.tensor([output_length(orig, new, v) for v in lengths], device=x.device)
        y = torch.where(torch.arange(y.shape[1], device=x.device)[None, :] < new_len[:, None], y, torch.zeros_like(y))
    return y


def rel_l2(got, want):
    """|got - want|_2 / |want|_2 in float64."""
    want = want.double()
    return ((got.double() - want).norm() / want.norm().clamp(min=1e-300)).item()


def signal(B, T, seed):
    """(B, T) float32 in about [-0.5, 0.5]: a few sines plus noise, every sample its own value."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64)[None, :]
    f = torch.rand(B, 3, generator=g, dtype=torch.float64) * 0.2 + 0.01
    x = sum(0.12 * torch.sin(2 * math.pi * f[:, i:i + 1] * t + i) for i in range(3))
    return (x + 0.05 * torch.randn(B, T, generator=g, dtype=torch.float64)).float()
