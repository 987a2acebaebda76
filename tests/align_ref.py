"""Two restatements of the monotonic alignment of DESIGN.md section 18, in numpy, from the definitions alone.

``align32`` does csrc/align.hip's adds and compares in its order, in float32: the kernel must equal it bit for bit in score,
durations and path.  ``align64`` is the optimum over the same float32 scores in float64.  ``brute_force`` enumerates every
admissible path of a small matrix."""
import itertools

import numpy as np

U = 2.0 ** -24


def _walk(adv, T, N):
    """The backtrack from (T-1, N-1) over the stored choices ``adv`` (T, N) bool: on the borders the walk ignores them (n = 0
    stays, n = t advances).  -> (durations (N,), path (T,)) int32."""
    path = np.zeros(T, dtype=np.int32)
    n = N - 1
    for t in range(T - 1, 0, -1):
        path[t] = n
        step = bool(adv[t, n])
        if n == 0:
            step = False
        elif n == t:
            step = True
        if step:
            n -= 1
    path[0] = n
    assert n == 0
    return np.bincount(path, minlength=N).astype(np.int32), path


def _align(scores, dtype):
    x = np.asarray(scores)
    assert x.dtype == np.float32 and x.ndim == 2
    T, N = x.shape
    assert 1 <= N <= T
    x = x.astype(dtype)
    ninf = dtype(-np.inf)
    q = np.full(N, ninf, dtype=dtype)
    q[0] = x[0, 0]
    adv = np.zeros((T, N), dtype=bool)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            stay = q
            move = np.concatenate([np.array([ninf], dtype=dtype), q[:-1]])
            adv[t] = move > stay                                            # the tie rule: staying wins
            q = (x[t] + np.where(adv[t], move, stay)).astype(dtype)         # one rounded add per cell
    dur, path = _walk(adv, T, N)
    return q[N - 1], dur, path


def align32(scores):
    """-> (score float32, durations (N,) int32, path (T,) int32): the kernel's arithmetic, bit for bit."""
    return _align(scores, np.float32)


def align64(scores):
    """-> (score float64, durations, path): the optimum over the float32 scores, adds in float64."""
    return _align(scores, np.float64)


def path_score(scores, path):
    """(the path's scores summed in float64, the sum of their magnitudes)."""
    v = np.asarray(scores, dtype=np.float64)[np.arange(len(path)), np.asarray(path)]
    return float(v.sum()), float(np.abs(v).sum())


def bound(T, S):
    """(T + 2) u S: DESIGN.md section 18.3."""
    return (T + 2) * U * S


def is_admissible(path, T, N):
    p = np.asarray(path)
    return len(p) == T and p[0] == 0 and p[-1] == N - 1 and bool(np.isin(np.diff(p), (0, 1)).all())


def brute_force(scores):
    """-> (the greatest float64 score over all admissible paths, the paths that reach it)."""
    x = np.asarray(scores, dtype=np.float64)
    T, N = x.shape
    best, argbest = -np.inf, []
    for ups in itertools.combinations(range(1, T), N - 1):                  # the frames at which the path advances
        path = np.zeros(T, dtype=np.int64)
        for t in ups:
            path[t:] += 1
        s = x[np.arange(T), path].sum()
        if s > best:
            best, argbest = s, [path]
        elif s == best:
            argbest.append(path)
    return best, argbest


def random_path(g, T, N):
    """A random admissible path (T,) int64."""
    ups = np.sort(g.choice(np.arange(1, T), size=N - 1, replace=False)) if N > 1 else np.array([], dtype=np.int64)
    path = np.zeros(T, dtype=np.int64)
    for t in ups:
        path[t:] += 1
    return path


def log_softmax_rows(g, T, N):
    z = g.randn(T, N) * 2.0
    z = z - z.max(axis=1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32)


def mixed_sign(g, T, N):
    return (g.randn(T, N) * 3.0).astype(np.float32)
