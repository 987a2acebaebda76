"""Restatements of the learned-aligner scores of DESIGN.md section 20, in numpy, from the definitions alone.

``scores64`` / ``grads64`` are the definitions in float64: d = sum_c (q - k)^2, z = -tau d, s = z - lse + logp, and the gradient
dz = g - p G.  ``scores32`` / ``grads32`` do what csrc/aligner.hip and csrc/aligner_rows.hip do, in float32 and in their order: the
products as fmaf chains over the reduction index ascending (what v_mfma_f32_32x32x2_f32 computes), z = tau (2 q.k - |k|^2), a
row's sums as 64 lane sums over the columns l, l + 64, .. and the xor butterfly 32 .. 1, dz = fmaf(-p, G, g), the column sums of
dz in float64 rounded once, dK = 2 tau fmaf(-cs, k, sum).  ``prior64`` is the beta-binomial log prior in float64 (lgamma),
``prior_exact`` the same for scaling 1 in rational arithmetic."""
import math
from fractions import Fraction

import numpy as np
import torch

U = 2.0 ** -24
NINF = -np.inf


# ---- float64 -----------------------------------------------------------------------------------------------------------------
def _dist64(q, k):
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    d = np.zeros((q.shape[0], k.shape[0]))
    for c in range(q.shape[1]):
        d += (q[:, c, None] - k[None, :, c]) ** 2
    return d


def _lse64(z):
    m = z.max(axis=1)
    return m + np.log(np.exp(z - m[:, None]).sum(axis=1))


def scores64(q, k, tau, logp=None):
    """-> dict: z (T, N) = -tau d, lse (T,) of z, lse_k (T,) = lse + tau |q_t|^2 (the logsumexp of tau (2 q.k - |k|^2), the one
    the kernels keep), p = exp(z - lse), s = z - lse + logp."""
    z = -float(tau) * _dist64(q, k)
    lse = _lse64(z)
    zl = z - lse[:, None]
    s = zl if logp is None else zl + np.asarray(logp, np.float64)
    return dict(z=z, lse=lse, lse_k=lse + float(tau) * (np.asarray(q, np.float64) ** 2).sum(axis=1), p=np.exp(zl), s=s)


def grads64(q, k, tau, g, keep_qnorm=False):
    """-> (dq, dk, dlogp) in float64 from g = dL/ds (T, N).  ``keep_qnorm`` forms the -2 tau q_t sum_n dz term as well."""
    q64, k64, g = np.asarray(q, np.float64), np.asarray(k, np.float64), np.asarray(g, np.float64)
    p = scores64(q, k, tau)["p"]
    dz = g - p * g.sum(axis=1)[:, None]
    dq = 2.0 * tau * (dz @ k64)
    if keep_qnorm:
        dq = dq - 2.0 * tau * q64 * dz.sum(axis=1)[:, None]
    dk = 2.0 * tau * (dz.T @ q64 - k64 * dz.sum(axis=0)[:, None])
    return dq, dk, g.copy()


# ---- float32, the kernels' order ---------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def chain(A, W):
    """out[m][n] = the fmaf chain over j ascending of A[m][j] W[n][j], from +0."""
    A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for j in range(A.shape[1]):
        acc = _fma(A[:, j, None], W[None, :, j], acc)
    return acc


def wave_sum(x):
    """Row sums of x (rows, n) float32 as a wave forms them: lane l adds the columns l, l + 64, .. ascending, then the xor
    butterfly 32, 16, .. 1."""
    x = np.asarray(x, np.float32)
    rows, n = x.shape
    v = np.zeros((rows, 64), np.float32)
    for j0 in range(0, n, 64):
        w = min(64, n - j0)
        v[:, :w] = v[:, :w] + x[:, j0:j0 + w]
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ m]
    return v[:, 0].copy()


def z32(q, k, tau):
    q, k = np.asarray(q, np.float32), np.asarray(k, np.float32)
    kn = np.zeros(k.shape[0], np.float32)
    for c in range(k.shape[1]):
        kn = _fma(k[:, c], k[:, c], kn)
    return (np.float32(tau) * (np.float32(2.0) * chain(q, k) - kn[None, :])).astype(np.float32)


def rows32(z, logp=None):
    """The forward row pass on float32 z (T, N) -> (lse (T,), s (T, N)) in float32."""
    z = np.asarray(z, np.float32)
    m = z.max(axis=1)
    lse = (m + np.log(wave_sum(np.exp(z - m[:, None])))).astype(np.float32)
    s = (z - lse[:, None]).astype(np.float32)
    if logp is not None:
        s = (s + np.asarray(logp, np.float32)).astype(np.float32)
    return lse, s


def rows64(z, logp=None):
    """The same in float64 on the same float32 z."""
    z = np.asarray(z, np.float64)
    lse = _lse64(z)
    s = z - lse[:, None]
    return lse, (s if logp is None else s + np.asarray(logp, np.float64))


def rows_bwd32(z, lse, g):
    """The backward row pass -> (dz (T, N), column sums (N,)) in float32."""
    z, lse, g = np.asarray(z, np.float32), np.asarray(lse, np.float32), np.asarray(g, np.float32)
    p = np.exp((z - lse[:, None]).astype(np.float32))
    dz = _fma(-p, wave_sum(g)[:, None], g)
    return dz, dz.astype(np.float64).sum(axis=0).astype(np.float32)


def rows_bwd64(z, lse, g):
    z, lse, g = np.asarray(z, np.float64), np.asarray(lse, np.float64), np.asarray(g, np.float64)
    dz = g - np.exp(z - lse[:, None]) * g.sum(axis=1)[:, None]
    return dz, dz.sum(axis=0)


def scores32(q, k, tau, logp=None):
    """-> dict z, lse_k, s in float32, in the kernels' order."""
    z = z32(q, k, tau)
    lse, s = rows32(z, logp)
    return dict(z=z, lse_k=lse, s=s)


def grads32(q, k, tau, g):
    q, k, g = np.asarray(q, np.float32), np.asarray(k, np.float32), np.asarray(g, np.float32)
    f = scores32(q, k, tau)
    dz, cs = rows_bwd32(f["z"], f["lse_k"], g)
    tau2 = np.float32(2.0) * np.float32(tau)
    dq = (tau2 * chain(dz, k.T)).astype(np.float32)
    dk = (tau2 * _fma(-cs[:, None], k, chain(dz.T, q.T))).astype(np.float32)
    return dq, dk, g.copy()


# ---- the prior -----------------------------------------------------------------------------------------------------------------
def prior64(T, N, scaling=1.0):
    """(T, N) float64: lgamma(m+1) - lgamma(n+1) - lgamma(m-n+1) + lbeta(n + a, m - n + b) - lbeta(a, b)."""
    lg = lambda x: torch.lgamma(torch.as_tensor(x, dtype=torch.float64)).numpy()      # noqa: E731
    t, n = np.arange(T, dtype=np.float64)[:, None], np.arange(N, dtype=np.float64)[None, :]
    a, b, m = scaling * (t + 1.0), scaling * (T - t), float(N - 1)
    choose = lg(m + 1.0) - lg(n + 1.0) - lg(m - n + 1.0)
    top = lg(n + a) + lg(m - n + b) - lg(m + a + b)
    bot = lg(a) + lg(b) - lg(a + b)
    return choose + top - bot


def prior_exact(T, N):
    """The prior of scaling 1 as exact rationals -> ((T, N) float64 of their logs, the T exact row sums)."""
    f = math.factorial
    beta = lambda x, y: Fraction(f(x - 1) * f(y - 1), f(x + y - 1))                   # noqa: E731
    out, sums = np.zeros((T, N)), []
    m = N - 1
    for t in range(T):
        a, b = t + 1, T - t
        row = [math.comb(m, n) * beta(n + a, m - n + b) / beta(a, b) for n in range(N)]
        sums.append(sum(row))
        out[t] = [math.log(v.numerator) - math.log(v.denominator) for v in row]
    return out, sums


# ---- tolerances (DESIGN.md sections 19.4 and 20.4) ---------------------------------------------------------------------------------
def allowed(v32, v64):
    """max(4 x the float32 restatement's own largest error, 8 2^-24 max(1, largest |value|)) over the finite values of v64."""
    v32, v64 = np.asarray(v32, np.float64), np.asarray(v64, np.float64)
    fin = np.isfinite(v64)
    if not fin.any():
        return 0.0
    return max(4.0 * float(np.abs(v32[fin] - v64[fin]).max()), 8 * U * max(1.0, float(np.abs(v64[fin]).max())))


def error(got, v64):
    """The largest absolute error over the finite values of v64; the others must be equal as they are."""
    got, v64 = np.asarray(got, np.float64), np.asarray(v64, np.float64)
    fin = np.isfinite(v64)
    assert np.array_equal(got[~fin], v64[~fin]), "non-finite values differ"
    assert np.isfinite(got[fin]).all(), "non-finite where a value was expected"
    return float(np.abs(got[fin] - v64[fin]).max()) if fin.any() else 0.0
