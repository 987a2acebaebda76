"""Restatements of the masked self-attention of DESIGN.md section 22, in numpy, from the definition alone, for one utterance and one
head: q, k, v, g are (T, D).

``forward64`` / ``backward64`` are the definition in float64.  ``forward32`` / ``backward32`` / ``delta32`` do what
csrc/self_attn.hip and csrc/self_attn_rows.hip do, in float32 and in their order: every product an fmaf chain over its reduction
index ascending (what v_mfma_f32_32x32x2_f32 computes), the scores scaled by one multiplication, the forward walking key tiles of
``bn`` keys with the online rescaling (m_new = max(m, tile max), alpha = exp(m - m_new), O scaled by alpha, the row sum kept as two
partial sums, one per parity of the key index, each fmaf(l, alpha, tile sum) with the tile sum over the keys ascending, added once at
the end), o = O / l, lse = m + log l; the backward with p = exp(scale s - lse), delta as 64 lane chains over d = l, l + 64 and the
xor butterfly 32 .. 1, ds = p (dp - delta), and scale applied once to the finished dq and dk sums.  numpy's float32 exp and log
stand in for the device's, which they cannot reproduce to the bit."""
import concurrent.futures
import os

import numpy as np

U = 2.0 ** -24


# ---- float64 -----------------------------------------------------------------------------------------------------------------
def forward64(q, k, v, scale):
    """-> dict: s (T, T), p, o (T, D), lse (T,)."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    s = float(scale) * (q @ k.T)
    m = s.max(axis=1)
    e = np.exp(s - m[:, None])
    l = e.sum(axis=1)
    p = e / l[:, None]
    return dict(s=s, p=p, o=p @ v, lse=m + np.log(l))


def backward64(q, k, v, g, scale):
    """-> dict: delta (T,), dq, dk, dv (T, D) from g = dL/do."""
    q, k, v, g = (np.asarray(x, np.float64) for x in (q, k, v, g))
    f = forward64(q, k, v, scale)
    delta = (g * f["o"]).sum(axis=1)
    ds = f["p"] * (g @ v.T - delta[:, None])
    return dict(delta=delta, dq=float(scale) * (ds @ k), dk=float(scale) * (ds.T @ q), dv=f["p"].T @ g)


# ---- float32, the kernels' order ---------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def chain(A, W):
    """out[m][n] = the fmaf chain over j ascending of A[m][j] W[n][j], from +0.  Blocks of rows, so that a block's accumulator
    stays in the cache, on a few threads (numpy releases the interpreter inside its loops); the rows do not meet, so neither
    changes a bit."""
    A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
    out = np.zeros((A.shape[0], W.shape[0]), np.float32)
    W64 = np.ascontiguousarray(W.astype(np.float64).T)                      # [j][n]
    rows = max(1, (1 << 20) // max(1, W.shape[0]))

    def block(r0):
        a64 = np.ascontiguousarray(A[r0:r0 + rows].astype(np.float64).T)    # [j][m]
        acc = np.zeros((a64.shape[1], W.shape[0]), np.float32)
        buf = np.empty(acc.shape, np.float64)
        for j in range(A.shape[1]):
            np.multiply(a64[j][:, None], W64[j][None, :], out=buf)
            np.add(buf, acc, out=buf)
            acc[...] = buf
        out[r0:r0 + rows] = acc

    starts = list(range(0, A.shape[0], rows))
    if len(starts) > 1:
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            list(pool.map(block, starts))
    else:
        for r0 in starts:
            block(r0)
    return out


def wave_sum(x):
    """The xor butterfly 32, 16, .. 1 over the last axis of 64 lanes: every lane ends with the same bits; lane 0's are returned."""
    x = np.asarray(x, np.float32)
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        x = x + x[..., idx ^ m]
    return x[..., 0]


def delta32(g, o):
    """delta (T,) of one head: lane l chains d = l, l + 64 ascending, then the butterfly."""
    g, o = np.asarray(g, np.float32), np.asarray(o, np.float32)
    T, D = g.shape
    lanes = np.zeros((T, 64), np.float32)
    for d0 in range(0, D, 64):
        w = min(64, D - d0)
        lanes[:, :w] = _fma(g[:, d0:d0 + w], o[:, d0:d0 + w], lanes[:, :w])
    return wave_sum(lanes)


def forward32(q, k, v, scale, bn=64):
    """-> dict: o (T, D), lse (T,) in float32, the forward kernel's order with key tiles of ``bn`` keys."""
    q, k, v = (np.asarray(x, np.float32) for x in (q, k, v))
    T, D = q.shape
    acc = chain(q, k)
    s = np.float32(scale) * acc
    m = np.full(T, -np.inf, np.float32)
    lpar = np.zeros((T, 2), np.float32)
    O = np.zeros((T, D), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j0 in range(0, T, bn):
            st = s[:, j0:j0 + bn]
            m_new = np.maximum(m, st.max(axis=1))
            alpha = np.exp(m - m_new)
            p = np.exp(st - m_new[:, None])
            for h in (0, 1):
                ps = np.zeros(T, np.float32)
                for c in range(h, p.shape[1], 2):
                    ps = ps + p[:, c]
                lpar[:, h] = _fma(lpar[:, h], alpha, ps)
            O = O * alpha[:, None]
            for c in range(p.shape[1]):
                O = _fma(v[None, j0 + c, :], p[:, c, None], O)
            m = m_new
    lt = lpar[:, 0] + lpar[:, 1]
    return dict(o=O / lt[:, None], lse=m + np.log(lt), qk=acc)


def backward32(q, k, v, o, lse, g, scale, qk=None):
    """-> dict: delta, dq, dk, dv in float32 from the float32 ``o`` and ``lse`` of ``forward32`` (``qk``: its score chain, which
    the backward kernels compute again to the same bits)."""
    q, k, v, o, lse, g = (np.asarray(x, np.float32) for x in (q, k, v, o, lse, g))
    sc = np.float32(scale)
    delta = delta32(g, o)
    p = np.exp(sc * (chain(q, k) if qk is None else qk) - lse[:, None])
    ds = p * (chain(g, v) - delta[:, None])
    return dict(delta=delta, dq=sc * chain(ds, k.T), dk=sc * chain(ds.T, q.T), dv=chain(p.T, g.T))


# ---- whole utterances (T, H, D) -----------------------------------------------------------------------------------------------
def _per_head(fn, arrays, names):
    H = arrays[0].shape[1]
    outs = [fn(*[np.ascontiguousarray(a[:, h]) for a in arrays]) for h in range(H)]
    res = {}
    for n in names:
        x = np.stack([o[n] for o in outs], axis=0)                          # (H, T, ..)
        res[n] = x if x.ndim == 2 else np.ascontiguousarray(np.transpose(x, (1, 0, 2)))
    return res


def attention64(q, k, v, g, scale):
    """-> dict of o, dq, dk, dv (T, H, D) and lse, delta (H, T) in float64."""
    def one(q_, k_, v_, g_):
        d = forward64(q_, k_, v_, scale)
        d.update(backward64(q_, k_, v_, g_, scale))
        return d
    return _per_head(one, (q, k, v, g), ("o", "lse", "delta", "dq", "dk", "dv"))


def attention32(q, k, v, g, scale, bn=64):
    def one(q_, k_, v_, g_):
        d = forward32(q_, k_, v_, scale, bn)
        d.update(backward32(q_, k_, v_, d["o"], d["lse"], g_, scale, d.pop("qk")))
        return d
    return _per_head(one, (q, k, v, g), ("o", "lse", "delta", "dq", "dk", "dv"))


def error(x, ref):
    return float(np.abs(np.asarray(x, np.float64) - ref).max()) if np.size(ref) else 0.0


def allowed(x32, x64):
    """max(4 x the float32 restatement's own error, 8 2^-24 max(1, largest |value|))."""
    return max(4.0 * error(x32, x64), 8.0 * U * max(1.0, float(np.abs(x64).max()) if np.size(x64) else 0.0))
