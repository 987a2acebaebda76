"""The thin projection and the thin embedding of a temporal predictor restated in numpy: in float64 (the
definition: each utterance alone, taps outside its own frames absent) and in float32 in the kernels' own orders:
  projection    lane l of 64 takes the float4 chunks l, l + 64, .. and chains fmaf(w, h, .) over their components from +0; the xor
                butterfly 32 .. 1; then bias + sum;
  dh            an fmaf chain from +0 over p ascending of g(t, p) w(p, c);
  embedding     an fmaf chain from +0 over p ascending, then j ascending, of w(c, p, j) v(t + j - k // 2, p), taps outside the
                utterance skipped; then bias + sum; then base + that;
  dv            u(t', p, j) = sum_c w(c, p, j) g(t', c) in the projection's order, dv(t, p) = the plain sum from +0 over j ascending
                of u(t - j + k // 2, p, j) over the rows inside the utterance;
  sums          P partial sums over runs of RP rows of the flattened (b, t) (``fft_block_ref.sum_plan``), fmaf for dw and plain
                adds for db, then the partial sums added ascending from +0.
All functions of one utterance take (T, .) arrays; the batch forms take lists."""
import numpy as np

from fft_block_ref import _lanes, image_dx, sum_plan, unfold
from self_attn_ref import U, _fma, allowed, error, wave_sum  # noqa: F401

F32 = np.float32


# ---- float64 -------------------------------------------------------------------------------------------------------------------
def project64(h, w, bias):
    y = h.astype(np.float64) @ w.astype(np.float64).T
    return y if bias is None else y + bias.astype(np.float64)


def project_bwd64(h, w, g):
    """-> dh (T, C), dw (P, C), db (P) of one utterance."""
    g = g.astype(np.float64)
    return g @ w.astype(np.float64), g.T @ h.astype(np.float64), g.sum(axis=0)


def _image(w):
    """[C][k P], tap-major, as ``unfold`` lays the tracks out."""
    return np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(w.shape[0], -1)


def embed64(v, w, bias, base):
    y = unfold(v.astype(np.float64), w.shape[2]) @ _image(w.astype(np.float64)).T
    if bias is not None:
        y = y + bias.astype(np.float64)
    return y if base is None else y + base.astype(np.float64)


def embed_bwd64(v, w, g):
    """-> dv (T, P), dw (C, P, k), db (C) of one utterance; dbase is g itself."""
    C, P, k = w.shape
    g = g.astype(np.float64)
    dv = unfold(g, k) @ image_dx(w.astype(np.float64)).T
    dw = (g.T @ unfold(v.astype(np.float64), k)).reshape(C, k, P).transpose(0, 2, 1)
    return dv, dw, g.sum(axis=0)


# ---- float32, the kernels' orders ----------------------------------------------------------------------------------------------
def lane_dot32(W, H):
    """(T, rows of W): the wave's dot product of every row of W (., C) with every row of H (T, C)."""
    W, H = np.asarray(W, F32), np.asarray(H, F32)
    T, C = H.shape
    q, ok = _lanes(C)
    H4 = H.reshape(T, C // 4, 4)
    out = np.zeros((T, len(W)), F32)
    for p, wrow in enumerate(W):
        w4 = wrow.reshape(C // 4, 4)
        s = np.zeros((T, 64), F32)
        for it in range(q.shape[0]):
            for c in range(4):
                s = np.where(ok[it][None, :], _fma(np.broadcast_to(w4[q[it], c][None, :], (T, 64)), H4[:, q[it], c], s), s)
        out[:, p] = wave_sum(s)
    return out


def project32(h, w, bias):
    s = lane_dot32(w, h)
    return s if bias is None else (bias.astype(F32)[None, :] + s).astype(F32)


def project_dh32(g, w):
    g, w = np.asarray(g, F32), np.asarray(w, F32)
    o = np.zeros((g.shape[0], w.shape[1]), F32)
    for p in range(w.shape[0]):
        o = _fma(np.broadcast_to(g[:, p:p + 1], o.shape), np.broadcast_to(w[p][None, :], o.shape), o)
    return o


def project_sums32(gs, hs, T_max):
    """(dw (P, C), db (P)) over a batch: ``gs`` the utterances' (T_b, P) gradients, ``hs`` their (T_b, C) inputs."""
    B, P, C = len(gs), gs[0].shape[1], hs[0].shape[1]
    parts, RP = sum_plan(B, T_max)
    s, s1 = np.zeros((parts, P, C), F32), np.zeros((parts, P), F32)
    for b, (g, h) in enumerate(zip(gs, hs)):
        for t in range(len(g)):
            n = (b * T_max + t) // RP
            for p in range(P):
                s[n, p] = _fma(np.broadcast_to(g[t, p], (C,)), h[t], s[n, p])
            s1[n] = s1[n] + g[t]
    dw, db = np.zeros((P, C), F32), np.zeros(P, F32)
    for n in range(parts):
        dw, db = dw + s[n], db + s1[n]
    return dw, db


def embed32(v, w, bias, base):
    v, w = np.asarray(v, F32), np.asarray(w, F32)
    T = v.shape[0]
    C, P, k = w.shape
    o = np.zeros((T, C), F32)
    for p in range(P):
        for j in range(k):
            off = j - k // 2
            lo, hi = max(0, -off), min(T, T - off)
            if hi > lo:
                o[lo:hi] = _fma(np.broadcast_to(w[:, p, j][None, :], (hi - lo, C)), np.broadcast_to(v[lo + off:hi + off, p:p + 1], (hi - lo, C)),
                                o[lo:hi])
    if bias is not None:
        o = (bias.astype(F32)[None, :] + o).astype(F32)
    return o if base is None else (base.astype(F32) + o).astype(F32)


def embed_dv32(g, w):
    g, w = np.asarray(g, F32), np.asarray(w, F32)
    T = g.shape[0]
    C, P, k = w.shape
    dv = np.zeros((T, P), F32)
    for p in range(P):
        for j in range(k):
            u = lane_dot32(w[:, p, j][None, :], g)[:, 0]
            off = k // 2 - j
            lo, hi = max(0, -off), min(T, T - off)
            if hi > lo:
                dv[lo:hi, p] = dv[lo:hi, p] + u[lo + off:hi + off]
    return dv


def embed_sums32(gs, vs, w_shape, T_max):
    """(dw (C, P, k), db (C)) over a batch: ``gs`` the utterances' (T_b, C) gradients, ``vs`` their (T_b, P) tracks."""
    C, P, k = w_shape
    parts, RP = sum_plan(len(gs), T_max)
    s = np.zeros((parts, P * k + 1, C), F32)
    for b, (g, v) in enumerate(zip(gs, vs)):
        T = len(g)
        for t in range(T):
            n = (b * T_max + t) // RP
            s[n, P * k] = s[n, P * k] + g[t]
            for p in range(P):
                for j in range(k):
                    tt = t + j - k // 2
                    if 0 <= tt < T:
                        s[n, p * k + j] = _fma(g[t], np.broadcast_to(v[tt, p], (C,)), s[n, p * k + j])
    total = np.zeros((P * k + 1, C), F32)
    for n in range(parts):
        total = total + s[n]
    return np.ascontiguousarray(total[:P * k].reshape(P, k, C).transpose(2, 0, 1)), total[P * k]
