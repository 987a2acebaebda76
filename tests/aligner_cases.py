"""The cases and assertions the CPU file (csrc/aligner_rows.hip on the host stand-in) and the GPU file (the MI355X) of the
learned-aligner tests share: every check takes a ``device`` and runs tacotron2_amd.native on tensors of that device.

Tolerance (DESIGN.md sections 19.4 and 20.4): per case and per tensor the largest absolute error against the float64 restatement
over the utterance's region is at most max(4 x the float32 restatement's own largest error on that case,
8 2^-24 max(1, largest |value| of that tensor in float64))."""
import ctypes
import functools

import numpy as np
import torch

import aligner_ref as ar
from tacotron2_amd import native

POISON, BPOISON = -777.0, 0xEE
SHAPES = [(1, 1, 1), (2, 2, 32), (7, 7, 80), (65, 64, 80), (129, 33, 96), (130, 127, 80), (257, 129, 160), (1030, 1024, 32),
          (4096, 5, 80)]
TAUS = (0.0005, 1.0)
ROW_SHAPES = [(1, 1), (2, 2), (7, 7), (9, 4), (17, 65), (33, 130)]          # the row kernels on the stand-in: (T, N)


def r32(n):
    return (n + 31) // 32 * 32


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def log_prior(g, T, N):
    """A normalised random log prior (T, N) float32."""
    x = g.randn(T, N) * 2.0
    x = x - x.max(axis=1, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(T, N, C, tau, prior, seed=0):
    """One utterance: q, k, logp (None without a prior), a random g, and both restatements of the scores, computed once."""
    g = np.random.RandomState(100000 * seed + 1000 * T + 10 * N + C)
    q, k = g.randn(T, C).astype(np.float32), g.randn(N, C).astype(np.float32)
    logp = log_prior(g, T, N) if prior else None
    grad = g.randn(T, N).astype(np.float32)
    for a in (q, k, logp, grad):
        if a is not None:
            a.setflags(write=False)
    return dict(T=T, N=N, C=C, tau=tau, q=q, k=k, logp=logp, g=grad, f32=ar.scores32(q, k, tau, logp), f64=ar.scores64(q, k, tau, logp))


def ragged_cases(tau=1.0):
    return [case(130, 65, 80, tau, True, 1), case(9, 1, 80, tau, True, 1), case(64, 64, 80, tau, False, 1), case(200, 31, 80, tau, True, 1),
            case(33, 40, 80, tau, False, 1), case(1, 1, 80, tau, True, 1)]


# ---- the whole path: native.aligner_scores / aligner_scores_backward -----------------------------------------------------------
def run(cases, device, offset=0, pad=3, grads=None, want_dlogp=True):
    """Forward and backward on poisoned outputs and poisoned workspaces for a ragged batch of cases of one C and tau.  The scores,
    the prior, the incoming gradient and the prior's gradient are views into wider buffers that start ``offset`` floats into their
    rows.  ``grads`` replaces the cases' own g.  -> dict of numpy arrays, after checking that the scores do not depend on whether
    anything is kept, that two calls agree bit for bit, the exact -inf and zeros of every utterance's padding, and that nothing was
    written outside the views."""
    B, C, tau = len(cases), cases[0]["C"], cases[0]["tau"]
    tl, nl = [c["T"] for c in cases], [c["N"] for c in cases]
    Tm, Nm = max(tl), max(nl)
    q, k = torch.full((B, Tm, C), 1e30), torch.full((B, Nm, C), 1e30)
    wide = (B, Tm + 1, offset + Nm + pad)
    lp, gbuf = torch.full(wide, 1e30), torch.full(wide, 1e30)
    has_prior = any(c["logp"] is not None for c in cases)
    for b, c in enumerate(cases):
        q[b, :tl[b]], k[b, :nl[b]] = torch.from_numpy(np.array(c["q"])), torch.from_numpy(np.array(c["k"]))
        lp[b, :tl[b], offset:offset + nl[b]] = 0.0 if c["logp"] is None else torch.from_numpy(np.array(c["logp"]))
        gbuf[b, :tl[b], offset:offset + nl[b]] = torch.from_numpy(np.array(c["g"] if grads is None else grads[b]))
    q, k = q.to(device), k.to(device)
    view = lambda t: t[:, :Tm, offset:offset + Nm]                          # noqa: E731
    lpv = view(lp.to(device)) if has_prior else None
    gv = view(gbuf.to(device))
    t_dev, n_dev = (torch.tensor(v, dtype=torch.int32).to(device) for v in (tl, nl))
    sizes = [native.aligner_workspace(B, Tm, Nm, C, w) for w in (0, 1, 2)]
    Cp, Np, Tp = r32(C), r32(Nm), r32(Tm)
    r4 = lambda n: (n + 3) // 4 * 4                                          # noqa: E731
    assert sizes[0] == 4 * B * Nm * Cp + 4 * r4(B * Nm) and sizes[1] == sizes[0] + 4 * r4(B * Tm)
    assert sizes[2] == 4 * B * Tm * Np + 4 * B * C * Np + 4 * B * C * Tp + 4 * r4(B * Nm)
    s0 = torch.full(wide, POISON, device=device)
    native.aligner_scores(q, k, t_dev, n_dev, tau, lpv, view(s0), torch.full((sizes[0],), BPOISON, dtype=torch.uint8, device=device), False)
    got = []
    for _ in range(2):
        sbuf, dlbuf = torch.full(wide, POISON, device=device), torch.full(wide, POISON, device=device)
        kept = torch.full((sizes[1],), BPOISON, dtype=torch.uint8, device=device)
        ws = torch.full((sizes[2],), BPOISON, dtype=torch.uint8, device=device)
        dq, dk = torch.full((B, Tm, C), POISON, device=device), torch.full((B, Nm, C), POISON, device=device)
        native.aligner_scores(q, k, t_dev, n_dev, tau, lpv, view(sbuf), kept, True)
        native.aligner_scores_backward(q, k, t_dev, n_dev, tau, gv, dq, dk, view(dlbuf) if want_dlogp else None, kept, ws)
        hs, hd = sbuf.cpu().numpy(), dlbuf.cpu().numpy()
        lse = kept.cpu().numpy()[sizes[0]:sizes[0] + 4 * B * Tm].view(np.float32).reshape(B, Tm)
        got.append(dict(s=view(hs).copy(), dlogp=view(hd).copy(), dq=dq.cpu().numpy(), dk=dk.cpu().numpy(), lse=lse.copy()))
        view(hs)[:] = POISON
        view(hd)[:] = POISON
        assert (hs == POISON).all() and (hd == POISON).all()               # nothing outside the views
        for b in range(B):
            assert (lse[b, tl[b]:].view(np.uint32) == 0xEEEEEEEE).all(), b       # lse is kept below T_b only
    one, two = got
    assert np.array_equal(bits(view(s0.cpu().numpy())), bits(one["s"]))
    for name in one:
        assert np.array_equal(bits(one[name]), bits(two[name])), name
    for b in range(B):
        T, N = tl[b], nl[b]
        assert (one["s"][b, T:] == -np.inf).all() and (one["s"][b, :, N:] == -np.inf).all(), b
        assert not one["dq"][b, T:].any() and not one["dk"][b, N:].any(), b
        if want_dlogp:
            assert not one["dlogp"][b, T:].any() and not one["dlogp"][b, :, N:].any(), b
    return one


def check_case(c, out, b=0, g=None, label=""):
    """Utterance b of ``out`` against the float64 restatement of case ``c`` within the allowed errors -> the ratios error / allowed."""
    T, N = c["T"], c["N"]
    g = c["g"] if g is None else g
    f32, f64 = c["f32"], c["f64"]
    want = ar.grads64(c["q"], c["k"], c["tau"], g)
    own = ar.grads32(c["q"], c["k"], c["tau"], g)
    pairs = [("s", out["s"][b, :T, :N], f32["s"], f64["s"]), ("lse", out["lse"][b, :T], f32["lse_k"], f64["lse_k"]),
             ("dq", out["dq"][b, :T], own[0], want[0]), ("dk", out["dk"][b, :N], own[1], want[1])]
    ratios = {}
    for name, got, v32, v64 in pairs:
        tol = ar.allowed(v32, v64)
        err = ar.error(got, v64)
        ratios[name] = err / tol
    assert np.array_equal(bits(out["dlogp"][b, :T, :N]), bits(np.asarray(g, np.float32))), "dlogp is g inside the utterance"
    if c["logp"] is None or np.isfinite(c["logp"]).all():              # exp(s - logp) is an attention map
        lp = 0.0 if c["logp"] is None else np.asarray(c["logp"], np.float64)
        rows = np.exp(out["s"][b, :T, :N].astype(np.float64) - lp).sum(axis=1)
        assert np.abs(rows - 1.0).max() <= 2 * ar.allowed(f32["s"], f64["s"]) + 1e-12, (T, N)
    print("FIGURE %s(%d, %d, %d) tau %g prior %s: error / allowed: %s"
          % (label, T, N, c["C"], c["tau"], c["logp"] is not None, ", ".join("%s %.4f" % kv for kv in ratios.items())))
    assert all(r <= 1.0 for r in ratios.values()), (T, N, c["C"], ratios)
    return ratios


def ragged_equals_alone(device):
    cases = ragged_cases()
    batch = run(cases, device, offset=1)
    for b, c in enumerate(cases):
        alone = run([c], device, offset=b % 3, pad=b)
        T, N = c["T"], c["N"]
        for name, rows in (("s", T), ("dlogp", T), ("dq", T), ("dk", N), ("lse", T)):
            a, o = batch[name][b, :rows], alone[name][0, :rows]
            if name in ("s", "dlogp"):
                a, o = a[:, :N], o[:, :N]
            assert np.array_equal(bits(a), bits(o)), (b, name)
        check_case(c, alone, label="alone ")


def many_short(device):
    """300 utterances: more workgroups than compute units."""
    g = np.random.RandomState(21)
    cases = [case(int(g.randint(1, 12)), int(g.randint(1, 12)), 32, 1.0, bool(i % 2), 2 + i) for i in range(300)]
    out = run(cases, device, offset=2)
    worst = {}
    for b, c in enumerate(cases):
        T, N = c["T"], c["N"]
        for name, got, v32, v64 in (("s", out["s"][b, :T, :N], c["f32"]["s"], c["f64"]["s"]),
                                    ("lse", out["lse"][b, :T], c["f32"]["lse_k"], c["f64"]["lse_k"])):
            worst[name] = max(worst.get(name, 0.0), ar.error(got, v64) / ar.allowed(v32, v64))
        assert np.array_equal(bits(out["dlogp"][b, :T, :N]), bits(c["g"])), b
        want, own = ar.grads64(c["q"], c["k"], 1.0, c["g"]), ar.grads32(c["q"], c["k"], 1.0, c["g"])
        worst["dq"] = max(worst.get("dq", 0.0), ar.error(out["dq"][b, :T], want[0]) / ar.allowed(own[0], want[0]))
        worst["dk"] = max(worst.get("dk", 0.0), ar.error(out["dk"][b, :N], want[1]) / ar.allowed(own[1], want[1]))
    print("FIGURE 300 utterances of 1 to 11 frames and tokens: worst error / allowed: %s" % ", ".join("%s %.4f" % kv for kv in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), worst


def ninf_column(device):
    """A -inf column in the prior: s = -inf there, everything else finite, the gradients as the float64 restatement has them."""
    c = dict(case(40, 17, 32, 1.0, True, 3))
    lp = np.array(c["logp"])
    lp[:, 9] = -np.inf
    c["logp"] = lp
    c["f32"], c["f64"] = ar.scores32(c["q"], c["k"], 1.0, lp), ar.scores64(c["q"], c["k"], 1.0, lp)
    out = run([c], device)
    assert (out["s"][0, :, 9] == -np.inf).all() and np.isfinite(np.delete(out["s"][0], 9, axis=1)).all()
    assert np.isfinite(out["dq"]).all() and np.isfinite(out["dk"]).all()
    check_case(c, out, label="-inf column ")


# ---- the row kernels alone (the stand-in runs these; the device can too) ------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _lib():
    return native.load()


def _ok(rc, lib):
    assert rc == 0, lib.t2amd_last_error()


def run_rows(mats, device, offset=0, pad=2, with_prior=True):
    """The three row kernels (and the packing kernels) on poisoned buffers for a ragged batch of (z (T, N), logp, g, k (N, C)):
    -> dict of numpy arrays, after two bit-identical calls and the padding checks."""
    lib = _lib()
    B = len(mats)
    tl, nl = [m[0].shape[0] for m in mats], [m[0].shape[1] for m in mats]
    Tm, Nm, C = max(tl), max(nl), mats[0][3].shape[1]
    Np, Cp = r32(Nm), r32(C)
    wide = (B, Tm + 1, offset + Nm + pad)
    sz, lp, gb = torch.full(wide, POISON), torch.full(wide, 1e30), torch.full(wide, 1e30)
    zslab = torch.full((B, Tm, Np), POISON)
    k = torch.full((B, Nm, C), 1e30)
    for b, (z, logp, g, kk) in enumerate(mats):
        sz[b, :tl[b], offset:offset + nl[b]] = torch.from_numpy(z)
        zslab[b, :tl[b], :nl[b]] = torch.from_numpy(z)
        lp[b, :tl[b], offset:offset + nl[b]] = torch.from_numpy(logp)
        gb[b, :tl[b], offset:offset + nl[b]] = torch.from_numpy(g)
        k[b, :nl[b]] = torch.from_numpy(kk)
    t_dev, n_dev = (torch.tensor(v, dtype=torch.int32).to(device) for v in (tl, nl))
    lp, gb, k = lp.to(device), gb.to(device), k.to(device)
    view = lambda t: t[:, :Tm, offset:offset + Nm]                          # noqa: E731
    st = wide[2]
    sb = wide[1] * st
    got = []
    for _ in range(2):
        s, dl = sz.clone().to(device), torch.full(wide, POISON, device=device)
        lse = torch.full((B, Tm), POISON, device=device)
        dz, cs = zslab.clone().to(device), torch.full((B, Nm), POISON, device=device)
        Kp, kn = torch.full((B, Nm, Cp), POISON, device=device), torch.full((B, Nm), POISON, device=device)
        KT = torch.full((B, C, Np), POISON, device=device)
        _ok(lib.t2amd_aligner_rows_fwd_f32(_p(view(s)), sb, st, _p(view(lp)) if with_prior else None, sb, st, _p(t_dev), _p(n_dev), B, Tm,
                                           Nm, _p(lse), None), lib)
        _ok(lib.t2amd_aligner_rows_bwd_f32(_p(view(gb)), sb, st, _p(t_dev), _p(n_dev), B, Tm, Nm, _p(lse), _p(dz), _p(cs), _p(view(dl)),
                                           sb, st, None), lib)
        _ok(lib.t2amd_aligner_pack_keys_f32(_p(k), _p(n_dev), B, Nm, C, _p(Kp), _p(kn), None), lib)
        _ok(lib.t2amd_aligner_transpose_f32(_p(k), _p(n_dev), B, Nm, C, _p(KT), None), lib)
        hs, hd = s.cpu().numpy(), dl.cpu().numpy()
        got.append(dict(s=view(hs).copy(), dlogp=view(hd).copy(), lse=lse.cpu().numpy(), dz=dz.cpu().numpy(), cs=cs.cpu().numpy(),
                        Kp=Kp.cpu().numpy(), kn=kn.cpu().numpy(), KT=KT.cpu().numpy()))
        view(hs)[:] = POISON
        view(hd)[:] = POISON
        assert (hs == POISON).all() and (hd == POISON).all()
    one, two = got
    for name in one:
        assert np.array_equal(bits(one[name]), bits(two[name])), name
    for b, (z, logp, g, kk) in enumerate(mats):
        T, N = tl[b], nl[b]
        assert (one["s"][b, T:] == -np.inf).all() and (one["s"][b, :, N:] == -np.inf).all() and (one["lse"][b, T:] == POISON).all(), b
        assert not one["dz"][b, T:].any() and not one["dz"][b, :, N:].any() and not one["cs"][b, N:].any(), b
        assert not one["dlogp"][b, T:].any() and not one["dlogp"][b, :, N:].any(), b
        assert np.array_equal(bits(one["dlogp"][b, :T, :N]), bits(g)), b
        assert np.array_equal(bits(one["Kp"][b, :N, :C]), bits(kk)) and not one["Kp"][b, N:].any() and not one["Kp"][b, :, C:].any(), b
        assert np.array_equal(bits(one["KT"][b, :, :N]), bits(kk.T)) and not one["KT"][b, :, N:].any() and not one["kn"][b, N:].any(), b
    return one


@functools.lru_cache(maxsize=None)
def row_mat(T, N, seed=0):
    g = np.random.RandomState(1000 * seed + 31 * T + N)
    z = (g.randn(T, N) * 3.0).astype(np.float32)
    return z, log_prior(g, T, N), g.randn(T, N).astype(np.float32), g.randn(N, 5).astype(np.float32)


def check_rows(mat, out, b=0, with_prior=True):
    z, logp, g, kk = mat
    T, N = z.shape
    lp = logp if with_prior else None
    (l32, s32), (l64, s64) = ar.rows32(z, lp), ar.rows64(z, lp)
    lse = out["lse"][b, :T]
    (dz32, cs32), (dz64, cs64) = ar.rows_bwd32(z, lse, g), ar.rows_bwd64(z, lse, g)
    kn64 = (kk.astype(np.float64) ** 2).sum(axis=1)
    kn32 = np.zeros(N, np.float32)
    for c in range(kk.shape[1]):
        kn32 = ar._fma(kk[:, c], kk[:, c], kn32)
    for name, got, v32, v64 in (("s", out["s"][b, :T, :N], s32, s64), ("lse", lse, l32, l64), ("dz", out["dz"][b, :T, :N], dz32, dz64),
                                ("cs", out["cs"][b, :N], cs32, cs64), ("kn", out["kn"][b, :N], kn32, kn64)):
        assert ar.error(got, v64) <= ar.allowed(v32, v64), (name, T, N)
    assert np.abs(np.exp(out["s"][b, :T, :N].astype(np.float64) - (logp if with_prior else 0.0)).sum(axis=1) - 1.0).max() <= 1e-5 * N


# ---- the prior -----------------------------------------------------------------------------------------------------------------
def check_prior(device, pairs, scaling, fn):
    """``fn(tl, nl, scaling, T, N, device)`` -> (B, T, N) tensor against ``prior64``: 4 2^-24 max(1, |logp|) per element, -inf in
    the padding, rows that sum to 1."""
    tl, nl = [p[0] for p in pairs], [p[1] for p in pairs]
    Tm, Nm = max(tl) + 1, max(nl) + 2
    out = fn(tl, nl, scaling, Tm, Nm, device)
    assert tuple(out.shape) == (len(pairs), Tm, Nm) and out.dtype == torch.float32 and not out.requires_grad
    h = out.cpu().numpy()
    worst = 0.0
    for b, (T, N) in enumerate(pairs):
        want = ar.prior64(T, N, scaling)
        assert (h[b, T:] == -np.inf).all() and (h[b, :, N:] == -np.inf).all(), b
        ratio = np.abs(h[b, :T, :N] - want) / (4 * ar.U * np.maximum(1.0, np.abs(want)))
        worst = max(worst, float(ratio.max()))
        assert np.abs(np.exp(h[b, :T, :N].astype(np.float64)).sum(axis=1) - 1.0).max() <= 1e-5
        if N == 1:
            assert not h[b, :T, 0].any()
    print("FIGURE prior scaling %g, %d utterances: worst error / allowed %.4f" % (scaling, len(pairs), worst))
    assert worst <= 1.0
    return h
