"""Restatements of the length regulator for the tests: the float64 one follows the definitions literally
(a Python loop over tokens); the float32 one follows the kernels' order (adds ascending from the first term, the fmaf chain from
+0, one division).  ``check_against_torch`` holds the float64 one to ``torch.repeat_interleave`` and float64 torch autograd."""
import itertools

import numpy as np
import torch

U = 2.0 ** -24


def gamma(k):
    """The constant of recursive summation: k u / (1 - k u)."""
    k = np.maximum(np.asarray(k, dtype=np.float64), 0.0)
    return k * U / (1.0 - k * U)


def path_of(d, n_len, T):
    """-> (path (T,) int32, T_b) of the definitions: Python integers, so no sum overflows."""
    d = [int(v) for v in list(d)[:n_len]]
    assert all(v >= 0 for v in d)
    Tb = min(sum(d), T)
    path = np.full(T, -1, dtype=np.int32)
    t = 0
    for n, run in enumerate(d):
        run = min(run, Tb - t)
        path[t:t + run] = n
        t += run
    return path, Tb


def expand(x, path):
    """y(t, :) = x(path(t), :), +0 where path is -1: a copy, so float32 in and out."""
    y = np.zeros((len(path), x.shape[1]), dtype=np.float32)
    y[path >= 0] = x[path[path >= 0]]
    return y


def _segments(path, N):
    """[(first frame, frames)] per token; (0, 0) for a token without one."""
    out = []
    for n in range(N):
        t = np.flatnonzero(path == n)
        out.append((int(t[0]), len(t)) if len(t) else (0, 0))
    return out


def segsum64(dy, path, N):
    """-> (dx in float64, sum of |dy| over the segment, frames of the segment (N,))."""
    dx, mag, cnt = (np.zeros((N, dy.shape[1])), np.zeros((N, dy.shape[1])), np.zeros(N, dtype=np.int64))
    for n, (t0, m) in enumerate(_segments(path, N)):
        seg = dy[t0:t0 + m].astype(np.float64)
        dx[n], mag[n], cnt[n] = seg.sum(axis=0), np.abs(seg).sum(axis=0), m
    return dx, mag, cnt


def segsum32(dy, path, N):
    dx = np.zeros((N, dy.shape[1]), dtype=np.float32)
    for n, (t0, m) in enumerate(_segments(path, N)):
        if m:
            s = dy[t0].copy()
            for t in range(t0 + 1, t0 + m):
                s = (s + dy[t]).astype(np.float32)
            dx[n] = s
    return dx


def fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to odd there (the error of
    the float64 add is known exactly), and 53 >= 2 * 24 + 2 bits make the second rounding the only one that counts."""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    s = np.where((err != 0) & ((bits & 1) == 0), other, s)
    return s.astype(np.float32)


def pool64(v, w, path, N):
    """-> dict of float64 arrays: num, den, m, and for the bound sum |w v| and the frames per token."""
    C = v.shape[1]
    out = dict(num=np.zeros((N, C)), den=np.zeros(N), m=np.zeros((N, C)), mag=np.zeros((N, C)), cnt=np.zeros(N, dtype=np.int64))
    for n, (t0, m) in enumerate(_segments(path, N)):
        ww, vv = w[t0:t0 + m].astype(np.float64), v[t0:t0 + m].astype(np.float64)
        out["num"][n], out["den"][n] = (ww[:, None] * vv).sum(axis=0), ww.sum()
        out["mag"][n], out["cnt"][n] = np.abs(ww[:, None] * vv).sum(axis=0), m
        if out["den"][n] > 0:
            out["m"][n] = out["num"][n] / out["den"][n]
    return out


def pool32(v, w, path, N):
    C = v.shape[1]
    num, den, mean = np.zeros((N, C), np.float32), np.zeros(N, np.float32), np.zeros((N, C), np.float32)
    for n, (t0, m) in enumerate(_segments(path, N)):
        s, dn = np.zeros(C, np.float32), np.float32(0)
        for t in range(t0, t0 + m):
            s = fma32(np.full(C, w[t], np.float32), v[t], s)
            dn = np.float32(dn + w[t])
        num[n], den[n] = s, dn
        if dn > 0:
            mean[n] = (s / dn).astype(np.float32)
    return dict(num=num, den=den, m=mean)


def pool_allowed(ref):
    """Section 21.4: |m - m64| <= 2 [(gamma_m sum |w v| + |m64| gamma_{m-1} sum w) / sum w + u |m64|], per element."""
    den = np.where(ref["den"] > 0, ref["den"], 1.0)[:, None]
    m = ref["cnt"][:, None]
    return 2.0 * ((gamma(m) * ref["mag"] + np.abs(ref["m"]) * gamma(m - 1) * den) / den + U * np.abs(ref["m"]))


def pool_bwd(g, den, w, path, dtype):
    """dv(t) = w(t) * (g(path(t)) / den(path(t))) in ``dtype``, +0 where den = 0 or path is -1."""
    g, den, w = g.astype(dtype), den.astype(dtype), w.astype(dtype)
    dv = np.zeros((len(path), g.shape[1]), dtype=dtype)
    for t, n in enumerate(path):
        if n >= 0 and den[n] > 0:
            dv[t] = (w[t] * (g[n] / den[n]).astype(dtype)).astype(dtype)
    return dv


def ulps(a, b):
    """The distance of two float32 arrays in units of the last place (finite values of one sign, or zeros)."""
    ia, ib = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7fffffff), i) for i in (ia, ib))
    return np.abs(ia - ib)


# ---- the float64 restatement against torch ------------------------------------------------------------------------------------
def _check_one(d, rng):
    N, S, C = len(d), int(sum(d)), 3
    x, w = rng.randn(N, C).astype(np.float32), rng.rand(max(S, 1)).astype(np.float32)[:S]
    path, Tb = path_of(d, N, S)
    assert Tb == S
    want = torch.repeat_interleave(torch.from_numpy(x), torch.tensor(d, dtype=torch.long), dim=0).numpy()
    assert np.array_equal(expand(x, path).view(np.int32), want.view(np.int32))
    assert np.array_equal(path, np.repeat(np.arange(N), d).astype(np.int32))
    if S == 0:
        return
    dy = rng.randn(S, C).astype(np.float32)
    leaf = torch.from_numpy(x).double().requires_grad_(True)
    (torch.repeat_interleave(leaf, torch.tensor(d, dtype=torch.long), dim=0) * torch.from_numpy(dy).double()).sum().backward()
    assert np.abs(segsum64(dy, path, N)[0] - leaf.grad.numpy()).max() <= 1e-12
    # pooling: a one-hot (S, N) matrix in float64 torch, and autograd through it
    v, g = rng.randn(S, C).astype(np.float32), rng.randn(N, C)
    hot = torch.zeros(S, N, dtype=torch.float64)
    hot[torch.arange(S), torch.from_numpy(path.astype(np.int64))] = 1.0
    vl, wt = torch.from_numpy(v).double().requires_grad_(True), torch.from_numpy(w).double()
    num, den = hot.t() @ (wt[:, None] * vl), hot.t() @ wt
    mean = torch.where(den[:, None] > 0, num / den.clamp_min(1e-300)[:, None], torch.zeros_like(num))
    ref = pool64(v, w, path, N)
    assert np.abs(ref["m"] - mean.detach().numpy()).max() <= 1e-12 and np.abs(ref["den"] - den.numpy()).max() <= 1e-12
    (mean * torch.from_numpy(g)).sum().backward()
    assert np.abs(pool_bwd(g, ref["den"], w, path, np.float64) - vl.grad.numpy()).max() <= 1e-12


def check_against_torch():
    """Every duration vector over {0, 1, 2, 3} up to 3 tokens, and random ones up to 9 tokens.  -> the count checked."""
    rng, count = np.random.RandomState(0), 0
    for N in (1, 2, 3):
        for d in itertools.product(range(4), repeat=N):
            _check_one(list(d), rng)
            count += 1
    for N in range(4, 10):
        for _ in range(6):
            _check_one([int(v) for v in rng.randint(0, 4, size=N)], rng)
            count += 1
    return count
