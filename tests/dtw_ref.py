"""The float64 restatement of mel-cepstral distortion under dynamic time warping in plain numpy, for the
tests and the bench only: the cepstrum as an explicit matrix, the cost matrix from differences, the recurrence with the tie rule
(the diagonal, then (i-1, j), then (i, j-1)), the step count carried with the cost, the backtrack and the MCD."""
import math

import numpy as np

MCD_DB = 10.0 / math.log(10.0) * math.sqrt(2.0)


def dct_matrix(n_mel, n_coef):
    """(n_coef, n_mel) float64, row k-1: sqrt(2 / N) cos(pi k (m + 1/2) / N), k = 1 ... n_coef, entry by entry."""
    M = np.zeros((n_coef, n_mel), dtype=np.float64)
    for k in range(1, n_coef + 1):
        for m in range(n_mel):
            M[k - 1, m] = math.sqrt(2.0 / n_mel) * math.cos(math.pi * k * (m + 0.5) / n_mel)
    return M


def cepstrum(mel, n_coef=13, lengths=None, basis=None):
    """mel (B, n_mel, T) -> (B, T, n_coef) float64; rows at and beyond ``lengths`` are zeros.  ``basis`` replaces the float64
    matrix (the float32-rounded one the kernel reads, as float64, for the error measurements)."""
    mel = np.asarray(mel, dtype=np.float64)
    M = dct_matrix(mel.shape[1], n_coef) if basis is None else np.asarray(basis, dtype=np.float64)
    c = np.einsum('km,bmt->btk', M, mel)
    if lengths is not None:
        for b, n in enumerate(lengths):
            c[b, n:] = 0.0
    return c


def cost_matrix(a, b):
    """a (n_a, K), b (n_b, K) -> (n_a, n_b) float64 Euclidean distances, differences first."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    df = a[:, None, :] - b[None, :, :]
    return np.sqrt((df * df).sum(axis=2))


def accumulate(d):
    """-> (D, N, choice): accumulated cost, cells of the chosen path and the chosen predecessor (0 diagonal, 1 (i-1, j),
    2 (i, j-1); 0 at the origin) of every cell."""
    n_a, n_b = d.shape
    D = np.full((n_a, n_b), np.inf)
    N = np.zeros((n_a, n_b), dtype=np.int64)
    ch = np.zeros((n_a, n_b), dtype=np.int64)
    for i in range(n_a):
        for j in range(n_b):
            if i == 0 and j == 0:
                D[0, 0], N[0, 0] = d[0, 0], 1
                continue
            best, bn, c = np.inf, 0, 0
            if i > 0 and j > 0:
                best, bn, c = D[i - 1, j - 1], N[i - 1, j - 1], 0
            if i > 0 and D[i - 1, j] < best:
                best, bn, c = D[i - 1, j], N[i - 1, j], 1
            if j > 0 and D[i, j - 1] < best:
                best, bn, c = D[i, j - 1], N[i, j - 1], 2
            D[i, j], N[i, j], ch[i, j] = d[i, j] + best, bn + 1, c
    return D, N, ch


def backtrack(ch):
    """The path the predecessor choices describe, forward, as a list of (i, j)."""
    i, j = ch.shape[0] - 1, ch.shape[1] - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        c = ch[i, j]
        if c != 2:
            i -= 1
        if c != 1:
            j -= 1
        path.append((i, j))
    return path[::-1]


def dtw(a, b):
    """-> (cost, steps, path) of the restatement for one pair."""
    D, N, ch = accumulate(cost_matrix(a, b))
    path = backtrack(ch)
    assert len(path) == N[-1, -1]
    return float(D[-1, -1]), int(N[-1, -1]), path


def mcd(cost, steps):
    return MCD_DB * cost / steps


def is_warping_path(path, n_a, n_b):
    """Starts at (0, 0), ends at (n_a - 1, n_b - 1), every step is one of (1, 1), (1, 0), (0, 1)."""
    path = [tuple(int(v) for v in p) for p in path]
    if not path or path[0] != (0, 0) or path[-1] != (n_a - 1, n_b - 1):
        return False
    for (i0, j0), (i1, j1) in zip(path[:-1], path[1:]):
        if (i1 - i0, j1 - j0) not in ((1, 1), (1, 0), (0, 1)):
            return False
    return True


def path_cost(a, b, path):
    """The sum of the local costs along ``path``, float64."""
    d = cost_matrix(a, b)
    return float(sum(d[int(i), int(j)] for i, j in path))


def unique_by_margin(a, b, rel=1e-3):
    """True when at every cell of the restatement's optimal path the best admissible predecessor beats the second best by at
    least ``rel`` times that cell's accumulated cost (cells with one admissible predecessor pass)."""
    D, _, ch = accumulate(cost_matrix(a, b))
    for i, j in backtrack(ch):
        cands = []
        if i > 0 and j > 0:
            cands.append(D[i - 1, j - 1])
        if i > 0:
            cands.append(D[i - 1, j])
        if j > 0:
            cands.append(D[i, j - 1])
        if len(cands) >= 2:
            cands.sort()
            if cands[1] - cands[0] < rel * D[i, j]:
                return False
    return True


def brute_force(d):
    """The minimum path cost over ALL warping paths by enumeration (tiny shapes only)."""
    n_a, n_b = d.shape

    def go(i, j):
        if i == n_a - 1 and j == n_b - 1:
            return d[i, j]
        best = np.inf
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < n_a and j + dj < n_b:
                best = min(best, go(i + di, j + dj))
        return d[i, j] + best
    return go(0, 0)


def bound(n_a, n_b, K):
    """The relative bound of the float32 kernel's cost against the float64 optimum over the same float32 inputs:
    (n_a + n_b + K + 8) 2^-24."""
    return (n_a + n_b + K + 8) * 2.0 ** -24


def sequences(n_a, n_b, K, seed):
    """Two float32 cepstrum-like sequences: a smooth random walk and a time-warped noisy copy of it."""
    g = np.random.RandomState(seed)
    base = np.cumsum(g.randn(max(n_a, n_b) + 4, K), axis=0) * 0.3 + g.randn(1, K)
    ia = np.linspace(0, base.shape[0] - 1, n_a) if n_a > 1 else np.array([0.0])
    ib = np.linspace(0, base.shape[0] - 1, n_b) ** 1.0 if n_b > 1 else np.array([1.0])
    a = np.stack([np.interp(ia, np.arange(base.shape[0]), base[:, k]) for k in range(K)], axis=1)
    b = np.stack([np.interp(ib, np.arange(base.shape[0]), base[:, k]) for k in range(K)], axis=1) + 0.1 * g.randn(n_b, K)
    return a.astype(np.float32), b.astype(np.float32)
