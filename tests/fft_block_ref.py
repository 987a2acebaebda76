"""The ragged convolution and add + LayerNorm of the feed-forward Transformer block restated in numpy: in
float64 (the definition: each utterance alone, zeros on both sides of its own frames) and in float32 in the kernels' own orders:
  convolution   an fmaf chain from +0 over K = (tap, channel) ascending, absent frames as zeros, then + bias, then ReLU;
  dx            the same on the flipped, transposed weights, after the gradient was multiplied by [y > 0];
  dw            the reduction index b Tp + t cut into S slices of L (``dw_plan``), a chain per slice, the slices added ascending;
  add + LN      lane l of 64 takes the float4 chunks l, l + 64, ..; sum (z0 + z1) + (z2 + z3) per chunk, the xor butterfly, / C;
                the variance an fmaf chain over the components, butterfly, / C; rstd = 1 / sqrt(var + eps);
  column sums   P partial sums over runs of RP rows of the flattened (b, t) (``sum_plan``), added ascending from +0.
All functions of one utterance take (T, C) arrays; the batch forms take lists."""
import numpy as np

from self_attn_ref import U, _fma, allowed, chain, error, wave_sum  # noqa: F401

F32 = np.float32


# ---- float64 -------------------------------------------------------------------------------------------------------------------
def unfold(x, k):
    """(T, k C): row t holds x[t + j - k // 2] for j = 0 .. k - 1, zeros where that frame does not exist."""
    T, C = x.shape
    out = np.zeros((T, k * C), x.dtype)
    for j in range(k):
        off = j - k // 2
        lo, hi = max(0, -off), min(T, T - off)
        if hi > lo:
            out[lo:hi, j * C:(j + 1) * C] = x[lo + off:hi + off]
    return out


def image(w):
    """[Cout][k Cin], tap-major."""
    return np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(w.shape[0], -1)


def image_dx(w):
    """[Cin][k Cout] of the flipped, transposed weights."""
    return np.ascontiguousarray(w[:, :, ::-1].transpose(1, 2, 0)).reshape(w.shape[1], -1)


def conv64(x, w, bias, relu):
    k = w.shape[2]
    y = unfold(x.astype(np.float64), k) @ image(w.astype(np.float64)).T
    if bias is not None:
        y = y + bias.astype(np.float64)
    return np.maximum(y, 0.0) if relu else y


def conv_bwd64(x, w, bias, relu, g):
    """-> dx (T, Cin), dw (Cout, Cin, k), dbias (Cout) of one utterance."""
    k = w.shape[2]
    g = g.astype(np.float64)
    if relu:
        g = g * (conv64(x, w, bias, True) > 0)
    dx = unfold(g, k) @ image_dx(w.astype(np.float64)).T
    dw = (g.T @ unfold(x.astype(np.float64), k)).reshape(w.shape[0], k, w.shape[1]).transpose(0, 2, 1)
    return dx, dw, g.sum(axis=0)


def add_ln64(x, res, w, b, eps):
    z = x.astype(np.float64) + (0 if res is None else res.astype(np.float64))
    mean = z.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((z - mean) ** 2).mean(axis=1, keepdims=True) + eps)
    return (z - mean) * rstd * w.astype(np.float64) + b.astype(np.float64)


def add_ln_bwd64(x, res, w, eps, g):
    """-> dz (T, C), dweight (C), dbias (C)."""
    z = x.astype(np.float64) + (0 if res is None else res.astype(np.float64))
    mean = z.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((z - mean) ** 2).mean(axis=1, keepdims=True) + eps)
    xh = (z - mean) * rstd
    gw = g.astype(np.float64) * w.astype(np.float64)
    dz = (gw - gw.mean(axis=1, keepdims=True) - xh * (gw * xh).mean(axis=1, keepdims=True)) * rstd
    return dz, (g.astype(np.float64) * xh).sum(axis=0), g.astype(np.float64).sum(axis=0)


# ---- float32, the kernels' orders ----------------------------------------------------------------------------------------------
def dw_plan(B, T):
    Tp = (T + 31) // 32 * 32
    K = B * Tp
    S = min(8, (K + 511) // 512)
    return Tp, S, ((K + S - 1) // S + 31) // 32 * 32


def sum_plan(B, T):
    rows = B * T
    P = min(64, (rows + 63) // 64)
    return P, (rows + P - 1) // P


def conv32(x, w, bias, relu):
    y = chain(unfold(x.astype(F32), w.shape[2]), image(w.astype(F32)))
    if bias is not None:
        y = y + bias.astype(F32)
    return np.maximum(y, F32(0)) if relu else y


def relu_mask32(g, y):
    return np.where(y > 0, g, F32(0)).astype(F32)


def dx32(g, w):
    return chain(unfold(g.astype(F32), w.shape[2]), image_dx(w.astype(F32)))


def dw32(gs, xs, w_shape, T_max):
    """dw of a batch: ``gs`` and ``xs`` the utterances' (T_b, Cout) masked gradients and (T_b, Cin) inputs."""
    Cout, Cin, k = w_shape
    Tp, S, L = dw_plan(len(gs), T_max)
    A = np.zeros((S * L, k * Cin), F32)
    G = np.zeros((S * L, Cout), F32)
    for b, (g, x) in enumerate(zip(gs, xs)):
        A[b * Tp:b * Tp + len(x)] = unfold(x.astype(F32), k)
        G[b * Tp:b * Tp + len(g)] = g
    total = None
    for s in range(S):
        part = chain(np.ascontiguousarray(A[s * L:(s + 1) * L].T), np.ascontiguousarray(G[s * L:(s + 1) * L].T))   # [k Cin][Cout]
        total = part if total is None else total + part
    return np.ascontiguousarray(total.reshape(k, Cin, Cout).transpose(2, 1, 0))


def colsum32(gs, T_max, xhs=None):
    """(dbias, dweight) over a batch: ``gs`` the utterances' (T_b, C) gradients, ``xhs`` their (z - mean) rstd or None."""
    B, C = len(gs), gs[0].shape[1]
    P, RP = sum_plan(B, T_max)
    s1, s2 = np.zeros((P, C), F32), np.zeros((P, C), F32)
    for b, g in enumerate(gs):
        for t in range(len(g)):
            p = (b * T_max + t) // RP
            s1[p] = s1[p] + g[t]
            if xhs is not None:
                s2[p] = _fma(g[t], xhs[b][t], s2[p])
    a1, a2 = np.zeros(C, F32), np.zeros(C, F32)
    for p in range(P):
        a1, a2 = a1 + s1[p], a2 + s2[p]
    return a1, a2


def _lanes(C):
    """The float4 chunks as (iteration, lane) with the padding marked: index arrays of shape (n_it, 64) and a validity mask."""
    nq = C // 4
    n_it = (nq + 63) // 64
    q = np.arange(n_it)[:, None] * 64 + np.arange(64)[None, :]
    return np.minimum(q, nq - 1), q < nq


def ln_stats32(z, eps):
    """-> mean (T,), rstd (T,) of (T, C) float32 rows in the kernel's order."""
    T, C = z.shape
    q, ok = _lanes(C)
    z4 = z.reshape(T, C // 4, 4)
    s = np.zeros((T, 64), F32)
    for it in range(q.shape[0]):
        a = z4[:, q[it]]                                                    # (T, 64, 4)
        add = (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])
        s = np.where(ok[it][None, :], s + add, s)
    mean = (wave_sum(s) / F32(C)).astype(F32)
    ss = np.zeros((T, 64), F32)
    for it in range(q.shape[0]):
        a = z4[:, q[it]]
        for c in range(4):
            d = a[..., c] - mean[:, None]
            ss = np.where(ok[it][None, :], _fma(d, d, ss), ss)
    rstd = (F32(1) / np.sqrt((wave_sum(ss) / F32(C)).astype(F32) + F32(eps))).astype(F32)
    return mean, rstd


def add_ln32(x, res, w, b, eps):
    """-> y, z, mean, rstd."""
    z = x.astype(F32) if res is None else x.astype(F32) + res.astype(F32)
    mean, rstd = ln_stats32(z, eps)
    xh = (z - mean[:, None]) * rstd[:, None]
    return _fma(xh, np.broadcast_to(w.astype(F32), xh.shape), np.broadcast_to(b.astype(F32), xh.shape)), z, mean, rstd


def add_ln_bwd32(g, z, mean, rstd, w):
    T, C = z.shape
    q, ok = _lanes(C)
    xh = (z - mean[:, None]) * rstd[:, None]
    gw = (g.astype(F32) * w.astype(F32)[None, :]).astype(F32)
    gw4, xh4 = gw.reshape(T, C // 4, 4), xh.reshape(T, C // 4, 4)
    s1, s2 = np.zeros((T, 64), F32), np.zeros((T, 64), F32)
    for it in range(q.shape[0]):
        for c in range(4):
            a, h = gw4[:, q[it], c], xh4[:, q[it], c]
            s1 = np.where(ok[it][None, :], s1 + a, s1)
            s2 = np.where(ok[it][None, :], _fma(a, h, s2), s2)
    m1, m2 = (wave_sum(s1) / F32(C)).astype(F32), (wave_sum(s2) / F32(C)).astype(F32)
    return (_fma(-xh, np.broadcast_to(m2[:, None], xh.shape), gw - m1[:, None]) * rstd[:, None]).astype(F32), xh
