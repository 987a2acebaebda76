"""Restatements of the forward-sum alignment likelihood of DESIGN.md section 19, in numpy, from the definitions alone.

``forward_sum64`` is alpha, beta, gamma, the soft durations and log Z in float64, nothing normalised.  ``forward_sum32`` does what
csrc/forward_sum.hip does, in float32 and in its order: every row relative to a float64 offset that takes the row's maximum,
logaddexp as max + log1p(exp(min - max)) (numpy's own formula for ``logaddexp``), the offset
A_t + B - log Z formed in float64 (log Z as it stood before it was rounded for the caller) and rounded once,
gamma = exp((alpha + beta) + offset), the soft durations summed in float64 from the last frame to the first and rounded once.  ``brute_force`` enumerates every admissible path of a small matrix."""
import itertools

import numpy as np

U = 2.0 ** -24
NINF = -np.inf


def forward_sum64(scores):
    """-> (log_z float64, gamma (T, N) float64, soft durations (N,) float64); zeros and -inf where no path is possible."""
    x = np.asarray(scores)
    assert x.dtype == np.float32 and x.ndim == 2
    T, N = x.shape
    assert 1 <= N <= T
    x = x.astype(np.float64)
    a = np.full((T, N), NINF)
    b = np.full((T, N), NINF)
    a[0, 0] = x[0, 0]
    b[T - 1, N - 1] = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(1, T):
            a[t] = x[t] + np.logaddexp(a[t - 1], np.concatenate([[NINF], a[t - 1, :-1]]))
        for t in range(T - 2, -1, -1):
            u = x[t + 1] + b[t + 1]
            b[t] = np.logaddexp(u, np.concatenate([u[1:], [NINF]]))
        log_z = a[T - 1, N - 1]
        if log_z == NINF:
            return log_z, np.zeros((T, N)), np.zeros(N)
        gamma = np.exp(a + b - log_z)
    return log_z, gamma, gamma.sum(axis=0)


def _logaddexp32(x, y):
    hi, lo = np.maximum(x, y), np.minimum(x, y)
    with np.errstate(invalid="ignore"):
        r = (hi + np.log1p(np.exp(lo - hi))).astype(np.float32)
    return np.where(hi == NINF, np.float32(NINF), r).astype(np.float32)


def _renormalise(row):
    m = row.max()
    m = np.float32(0.0) if m == NINF else m
    return (row - m).astype(np.float32), np.float64(m)


def forward_sum32(scores):
    """-> (log_z float32, gamma (T, N) float32, soft durations (N,) float32): the kernel's scheme in the kernel's order."""
    x = np.asarray(scores)
    assert x.dtype == np.float32 and x.ndim == 2
    T, N = x.shape
    assert 1 <= N <= T
    ninf = np.float32(NINF)
    a = np.full(N, ninf, dtype=np.float32)
    a[0] = x[0, 0]
    A = np.float64(0.0)
    keep = np.empty((T, N), np.float32)
    offs = np.empty(T, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            a, m = _renormalise(a)
            A = A + m
            keep[t], offs[t] = a, A
            if t + 1 < T:
                a = (x[t + 1] + _logaddexp32(a, np.concatenate([[ninf], a[:-1]]).astype(np.float32))).astype(np.float32)
        log_zd = A + np.float64(a[N - 1])
        log_z = np.float32(log_zd)
        gamma = np.zeros((T, N), np.float32)
        soft = np.zeros(N, np.float64)
        if log_z == ninf:
            return log_z, gamma, soft.astype(np.float32)
        b = np.full(N, ninf, dtype=np.float32)
        b[N - 1] = 0.0
        Bo = np.float64(0.0)
        for t in range(T - 1, -1, -1):
            b, m = _renormalise(b)
            Bo = Bo + m
            off = np.float32(offs[t] + Bo - log_zd)
            gamma[t] = np.exp(((keep[t] + b).astype(np.float32) + off).astype(np.float32))
            soft = soft + gamma[t]
            if t > 0:
                u = (x[t] + b).astype(np.float32)
                b = _logaddexp32(u, np.concatenate([u[1:], [ninf]]).astype(np.float32))
    return log_z, gamma, soft.astype(np.float32)


def brute_force(scores):
    """-> (log Z, gamma (T, N)) in float64 by enumerating every admissible path."""
    x = np.asarray(scores, dtype=np.float64)
    T, N = x.shape
    paths, sums = [], []
    for ups in itertools.combinations(range(1, T), N - 1):                  # the frames at which the path advances
        path = np.zeros(T, dtype=np.int64)
        for t in ups:
            path[t:] += 1
        paths.append(path)
        sums.append(x[np.arange(T), path].sum())
    sums = np.array(sums)
    top = sums.max()
    if top == NINF:
        return NINF, np.zeros((T, N))
    log_z = top + np.log(np.exp(sums - top).sum())
    gamma = np.zeros((T, N))
    for p, s in zip(paths, sums):
        gamma[np.arange(T), p] += np.exp(s - log_z)
    return log_z, gamma


def in_band(T, N):
    """(T, N) bool: the cells an admissible path can visit, n <= t and N - 1 - n <= T - 1 - t."""
    t, n = np.arange(T)[:, None], np.arange(N)[None, :]
    return (n <= t) & (N - 1 - n <= T - 1 - t)
