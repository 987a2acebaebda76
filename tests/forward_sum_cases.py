"""The cases and assertions the CPU file (csrc/forward_sum.hip on the host stand-in) and the GPU file (the MI355X) of the
forward-sum tests share: every check takes a ``device`` and runs tacotron2_amd.native / tacotron2_amd.alignment on tensors of that
device.

Tolerance: per case the allowed error of log Z, of gamma (largest absolute) and of the soft durations
against the float64 restatement is 4 x the float32 restatement's own error on that case, and at least 8 2^-24 max(1, |log Z|) for
log Z and 8 2^-24 for gamma and the durations.  The factor 4 stands for exp / log1p of the device differing from numpy's by a few
ulp; it is not a measurement."""
import functools
import math

import numpy as np
import torch

import align_ref as ar
import forward_sum_ref as fr
from tacotron2_amd import alignment, native

W = 256
POISON, BPOISON = -777.0, 0xEE
SHAPES = [(1, 1), (2, 1), (2, 2), (9, 1), (7, 7), (65, 64), (130, 63), (130, 65), (257, 255), (259, 256), (296, 257), (1030, 1024),
          (4096, 5)]
KINDS = ("log_softmax", "mixed_sign")
FLOOR = 8 * fr.U


@functools.lru_cache(maxsize=None)
def matrix(T, N, kind, seed=0):
    """(scores, the float32 restatement's result, the float64 one's) of one case, computed once."""
    g = np.random.RandomState(1000 * seed + 7 * T + N)
    x = ar.log_softmax_rows(g, T, N) if kind == "log_softmax" else ar.mixed_sign(g, T, N)
    x.setflags(write=False)
    return x, fr.forward_sum32(x), fr.forward_sum64(x)


def allowed(ref32, ref64):
    """The allowed errors (log Z, gamma, durations) of one case: 4 x the float32 restatement's own, with the floors."""
    z32, g32, d32 = ref32
    z64, g64, d64 = ref64
    if z64 == -np.inf:
        return 0.0, 0.0, 0.0
    return (max(4 * abs(float(z32) - z64), FLOOR * max(1.0, abs(z64))), max(4 * float(np.abs(g32 - g64).max()), FLOOR),
            max(4 * float(np.abs(d32 - d64).max()), FLOOR))


def _round4(n):
    return (n + 3) // 4 * 4


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def run(mats, device, offset=0, pad=3, scale=None):
    """The two native launches on poisoned outputs and a poisoned workspace for a ragged batch of (T, N) float32 matrices.  The
    batch is a view into a wider buffer that starts ``offset`` floats into its rows and holds 1e30 wherever no utterance is; the
    gradient goes to such a view as well.  -> (log_z, gamma, soft durations) as numpy, after checking that log Z does not depend
    on whether the rows are kept, that two calls agree bit for bit, with and without the durations, the zeros of every utterance's
    padding and outside its band, and that nothing was written outside an utterance's own region of any buffer."""
    B = len(mats)
    tl, nl = [m.shape[0] for m in mats], [m.shape[1] for m in mats]
    Tm, Nm = max(tl), max(nl)
    buf = torch.full((B, Tm + 1, offset + Nm + pad), 1e30)
    for b, m in enumerate(mats):
        buf[b, :tl[b], offset:offset + nl[b]] = torch.from_numpy(np.array(m))
    x = buf.to(device)[:, :Tm, offset:offset + Nm]
    t_dev, n_dev = (torch.tensor(v, dtype=torch.int32).to(device) for v in (tl, nl))
    sc = None if scale is None else torch.tensor(scale, dtype=torch.float32).to(device)
    small, nbytes = native.forward_sum_workspace(B, Tm, Nm, False), native.forward_sum_workspace(B, Tm, Nm, True)
    ld = _round4(Nm)
    assert small == 16 * B and nbytes == 4 * B * Tm * ld + 8 * B * Tm + 16 * B
    z0 = torch.full((B,), POISON, device=device)
    ws0 = torch.full((small,), BPOISON, dtype=torch.uint8, device=device)
    native.forward_sum(x, t_dev, n_dev, z0, ws0, False)
    got = []
    for with_soft in (False, True):
        z = torch.full((B,), POISON, device=device)
        ws = torch.full((nbytes,), BPOISON, dtype=torch.uint8, device=device)
        gbuf = torch.full((B, Tm + 1, offset + Nm + pad), POISON, device=device)
        soft = torch.full((B, Nm), POISON, device=device) if with_soft else None
        native.forward_sum(x, t_dev, n_dev, z, ws, True)
        native.forward_sum_backward(x, t_dev, n_dev, z, sc, gbuf[:, :Tm, offset:offset + Nm], soft, ws)
        h = gbuf.cpu().numpy()
        got.append((z.cpu().numpy(), h[:, :Tm, offset:offset + Nm].copy(), None if soft is None else soft.cpu().numpy()))
        h[:, :Tm, offset:offset + Nm] = POISON
        assert (h == POISON).all()                                          # nothing outside the gradient's own view
        raw = ws.cpu().numpy()
        slab = raw[:4 * B * Tm * ld].reshape(B, Tm, ld, 4)
        offs = raw[4 * B * Tm * ld:4 * B * Tm * ld + 8 * B * Tm].reshape(B, Tm, 8)
        for b in range(B):
            cols = nl[b] if Nm <= W else _round4(nl[b])                     # a lane of the four-column form stores its four at once
            assert (slab[b, tl[b]:] == BPOISON).all() and (slab[b, :, cols:] == BPOISON).all(), b
            assert (offs[b, tl[b]:] == BPOISON).all(), b
        assert (raw[-16 * B:].view(np.uint64) < 2 ** 40).all()              # the two clock counts: written, and no poison
    (z1, g1, _), (z, gamma, soft) = got
    assert np.array_equal(_bits(z0.cpu().numpy()), _bits(z)) and np.array_equal(_bits(z1), _bits(z)) and np.array_equal(_bits(g1), _bits(gamma))
    for b in range(B):
        T, N = tl[b], nl[b]
        assert not gamma[b, T:].any() and not gamma[b, :, N:].any() and not soft[b, N:].any(), b
        if not (np.isnan(mats[b]) | (np.asarray(mats[b]) == np.inf)).any():
            assert not gamma[b, :T, :N][~fr.in_band(T, N)].any(), b         # exact zeros outside the band
    return z, gamma, soft


def check_matrix(x, ref32, ref64, z, gamma, soft):
    """One utterance against the float64 restatement within the allowed errors.  -> the three ratios error / allowed."""
    T, N = x.shape
    z64, g64, d64 = ref64
    if z64 == -np.inf:
        assert z == -np.inf and not gamma[:T, :N].any() and not soft[:N].any()
        return 0.0, 0.0, 0.0
    tz, tg, td = allowed(ref32, ref64)
    ez, eg, ed = abs(float(z) - z64), float(np.abs(gamma[:T, :N] - g64).max()), float(np.abs(soft[:N] - d64).max())
    assert np.isfinite(gamma).all() and np.isfinite(soft).all()
    assert ez <= tz and eg <= tg and ed <= td, (T, N, (ez, tz), (eg, tg), (ed, td))
    rows = gamma[:T, :N].astype(np.float64).sum(axis=1)
    assert np.abs(rows - 1.0).max() <= tg * N and abs(float(soft[:N].astype(np.float64).sum()) - T) <= td * N, (T, N)
    return ez / tz, eg / tg, ed / td


def check_shape(T, N, kind, device, viterbi=None):
    x, ref32, ref64 = matrix(T, N, kind)
    z, gamma, soft = run([x], device, offset=(T + N) % 3)
    rz, rg, rd = check_matrix(x, ref32, ref64, z[0], gamma[0], soft[0])
    tz, tg, td = allowed(ref32, ref64)
    print("FIGURE %s (%d, %d): log Z %.6f, float64 %.6f; error / allowed: log Z %.4f (allowed %.3g), gamma %.4f (%.3g), "
          "durations %.4f (%.3g)" % (kind, T, N, float(z[0]), ref64[0], rz, tz, rg, tg, rd, td))
    if viterbi is not None:                                                 # section 18's best path is one of the paths summed
        score = float(viterbi(x))
        assert score <= float(z[0]) + tz + ar.bound(T, abs(score)), (T, N, score, float(z[0]))


def ragged_mats():
    g = np.random.RandomState(5)
    return [ar.log_softmax_rows(g, 130, 65), ar.mixed_sign(g, 9, 1), ar.mixed_sign(g, 64, 64), ar.log_softmax_rows(g, 200, 31),
            np.zeros((77, 12), np.float32), ar.mixed_sign(g, 1, 1)]


def ragged_equals_alone(mats, device):
    """A ragged batch gives each utterance the bits it gives alone (at another buffer stride), and a per-utterance scale scales."""
    scale = [1.0 + 0.5 * b for b in range(len(mats))]
    one = run(mats, device, offset=1)
    scaled = run(mats, device, offset=1, scale=scale)
    assert np.array_equal(_bits(one[0]), _bits(scaled[0])) and np.array_equal(_bits(one[2]), _bits(scaled[2]))
    for b, m in enumerate(mats):
        T, N = m.shape
        z, gamma, soft = run([m], device, offset=b % 3, pad=b)
        assert _bits(one[0])[b] == _bits(z)[0] and np.array_equal(_bits(one[1][b, :T, :N]), _bits(gamma[0])), b
        assert np.array_equal(_bits(one[2][b, :N]), _bits(soft[0])), b
        assert np.array_equal(_bits(scaled[1][b, :T, :N]), _bits(np.float32(scale[b]) * gamma[0])), b
        check_matrix(m, fr.forward_sum32(m), fr.forward_sum64(m), z[0], gamma[0], soft[0])


def many_short(device):
    """300 utterances: more workgroups than compute units."""
    g = np.random.RandomState(21)
    mats = []
    for _ in range(300):
        T = int(g.randint(1, 12))
        mats.append(ar.mixed_sign(g, T, int(g.randint(1, T + 1))))
    z, gamma, soft = run(mats, device, offset=2)
    worst = np.zeros(3)
    for b, m in enumerate(mats):
        worst = np.maximum(worst, check_matrix(m, fr.forward_sum32(m), fr.forward_sum64(m), z[b], gamma[b], soft[b]))
    print("FIGURE 300 utterances of 1 to 11 frames: worst error / allowed: log Z %.4f, gamma %.4f, durations %.4f" % tuple(worst))


def planted(device):
    """A random admissible path raised by 30 over noise in [-1, 0]: the posterior sits on it."""
    g = np.random.RandomState(11)
    for T, N in ((40, 40), (300, 97), (600, 300)):
        want = ar.random_path(g, T, N)
        x = -g.rand(T, N).astype(np.float32)
        x[np.arange(T), want] += np.float32(30.0)
        _, gamma, soft = run([x], device)
        assert (gamma[0][np.arange(T), want] >= 0.99).all(), (T, N)
        assert np.abs(soft[0] - np.bincount(want, minlength=N)).max() <= 0.05, (T, N)


def all_zero(device):
    """All-zero scores: every path has probability 1, log Z = log C(T-1, N-1)."""
    for T, N in ((1, 1), (5, 5), (9, 4), (W + 9, W + 2), (300, 7)):
        x = np.zeros((T, N), np.float32)
        z, gamma, soft = run([x], device)
        want = math.lgamma(T) - math.lgamma(N) - math.lgamma(T - N + 1)
        tz, _, _ = allowed(fr.forward_sum32(x), fr.forward_sum64(x))
        assert abs(fr.forward_sum64(x)[0] - want) <= 1e-9 * max(1.0, want) and abs(float(z[0]) - want) <= tz + 1e-9 * max(1.0, want), (T, N)
        check_matrix(x, fr.forward_sum32(x), fr.forward_sum64(x), z[0], gamma[0], soft[0])


def impossible(device):
    """-inf scores: a column of them leaves no path (log Z = -inf, zeros, no NaN); off the path everything stays finite."""
    g = np.random.RandomState(17)
    x = ar.mixed_sign(g, 40, 17)
    x[:, 9] = -np.inf
    y = np.full((30, 30), -np.inf, np.float32)
    w = ar.log_softmax_rows(g, 300, 260)
    w[:, 100] = -np.inf
    z, gamma, soft = run([x, y, ar.mixed_sign(g, 20, 3)], device)
    assert z[0] == -np.inf and z[1] == -np.inf and np.isfinite(z[2]) and not gamma[:2].any() and not soft[:2].any()
    assert not np.isnan(gamma).any() and not np.isnan(soft).any() and abs(soft[2].sum() - 20) < 1e-3
    z, gamma, soft = run([w], device)
    assert z[0] == -np.inf and not gamma.any() and not soft.any()
    for T, N in ((40, 17), (300, 260)):
        v = ar.mixed_sign(g, T, N)
        keep = ar.random_path(g, T, N)
        hole = g.rand(T, N) < 0.3
        hole[np.arange(T), keep] = False
        v[hole] = -np.inf
        z, gamma, soft = run([v], device)
        assert np.isfinite(z).all() and np.isfinite(gamma).all() and np.isfinite(soft).all() and not gamma[0][hole].any()
        check_matrix(v, fr.forward_sum32(v), fr.forward_sum64(v), z[0], gamma[0], soft[0])


def non_finite(device):
    """NaN and +inf scores give unspecified values, but ``run`` still finds every poison where it was."""
    g = np.random.RandomState(9)
    x = ar.mixed_sign(g, 40, 17)
    x[g.rand(40, 17) < 0.2] = np.nan
    x[g.rand(40, 17) < 0.2] = np.inf
    run([x, np.full((30, 30), -np.inf, np.float32)], device)


def _padded(mats, device, extra_t=2, extra_n=3):
    tl, nl = [m.shape[0] for m in mats], [m.shape[1] for m in mats]
    x = torch.zeros(len(mats), max(tl) + extra_t, max(nl) + extra_n)
    for b, m in enumerate(mats):
        x[b, :tl[b], :nl[b]] = torch.from_numpy(m)
    return x.to(device), tl, nl


def module_equals_native(mats, device):
    """alignment.forward_sum / alignment_posterior on the padded batch: the bits of the native calls at the buffer's own size; a
    (T, N) matrix is a batch of one; the gradient is gamma bit for bit and a non-unit grad_output scales it."""
    z, gamma, soft = run(mats, device)
    x, tl, nl = _padded(mats, device)
    Tm, Nm = max(tl), max(nl)
    g, d, lz = alignment.alignment_posterior(x, tl, nl)
    assert g.shape == x.shape and d.shape == (len(mats), Nm + 3) and lz.shape == (len(mats),)
    assert all(t.grad_fn is None and not t.requires_grad and t.dtype == torch.float32 for t in (g, d, lz))
    hg, hd = g.cpu().numpy(), d.cpu().numpy()
    assert np.array_equal(_bits(hg[:, :Tm, :Nm]), _bits(gamma)) and not hg[:, Tm:].any() and not hg[:, :, Nm:].any()
    assert np.array_equal(_bits(hd[:, :Nm]), _bits(soft)) and not hd[:, Nm:].any() and np.array_equal(_bits(lz.cpu().numpy()), _bits(z))
    plain = alignment.forward_sum(x, torch.tensor(tl), torch.tensor(nl))
    assert plain.grad_fn is None and torch.equal(plain, lz)
    leaf = x.clone().requires_grad_(True)
    out = alignment.forward_sum(leaf, tl, nl)
    assert out.grad_fn is not None and torch.equal(out.detach(), lz)
    out.sum().backward()
    assert leaf.grad.shape == x.shape and np.array_equal(_bits(leaf.grad.cpu().numpy()), _bits(hg))
    with torch.no_grad():
        assert alignment.forward_sum(leaf, tl, nl).grad_fn is None
    scale = torch.tensor([0.5 - b for b in range(len(mats))], dtype=torch.float32)
    leaf2 = x.clone().requires_grad_(True)
    (alignment.forward_sum(leaf2, tl, nl) * scale.to(device)).sum().backward()
    assert np.array_equal(leaf2.grad.cpu().numpy(), scale.numpy()[:, None, None] * hg)       # (as values: the padding is +0, not -0)
    one = x[0, :tl[0], :nl[0]].clone().requires_grad_(True)
    single = alignment.forward_sum(one)
    assert single.shape == (1,) and _bits(single.detach().cpu().numpy())[0] == _bits(z)[0]
    single.sum().backward()
    assert one.grad.shape == (tl[0], nl[0]) and np.array_equal(_bits(one.grad.cpu().numpy()), _bits(gamma[0, :tl[0], :nl[0]]))


def loss_module(mats, device):
    """ForwardSumLoss is -log Z, per frame and reduced as asked, and nothing else."""
    x, tl, nl = _padded(mats, device)
    lz = alignment.forward_sum(x, tl, nl).cpu()
    frames = torch.tensor(tl, dtype=torch.float32)
    for reduction, per_frame, want in (("none", False, -lz), ("sum", False, (-lz).sum()), ("mean", False, (-lz).mean()),
                                       ("none", True, -lz / frames), ("mean", True, (-lz / frames).mean())):
        got = alignment.ForwardSumLoss(reduction, per_frame)(x, tl, nl).cpu()
        assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-6, atol=0), (reduction, per_frame)
    import pytest
    with pytest.raises(ValueError, match="reduction"):
        alignment.ForwardSumLoss("max")
    assert not list(alignment.ForwardSumLoss().parameters())


def refusals(device):
    """The refusals of ``monotonic_align``, under the prefix ``forward_sum:``, from all three entry points."""
    import pytest
    x = torch.zeros(2, 6, 4).to(device)
    for fn in (alignment.forward_sum, alignment.alignment_posterior, alignment.ForwardSumLoss()):
        with pytest.raises(ValueError, match="forward_sum: utterance 1 has 4 tokens and only 3 frames"):
            fn(x, [6, 3], [4, 4])
        with pytest.raises(ValueError, match=r"forward_sum: utterance 0: 0 frames and 1 tokens do not lie in \[1, 6\] and \[1, 4\]"):
            fn(x, [0, 3], [1, 1])
        with pytest.raises(ValueError, match="forward_sum: utterance 1: 3 frames and 0 tokens do not lie"):
            fn(x, [6, 3], [4, 0])
        with pytest.raises(ValueError, match="forward_sum: utterance 1: 7 frames and 1 tokens do not lie"):
            fn(x, [6, 7], [4, 1])
        with pytest.raises(ValueError, match="forward_sum: utterance 0 has 4 tokens and only 3 frames"):
            fn(torch.zeros(3, 4).to(device))
        with pytest.raises(ValueError, match="forward_sum: utterance 0: 4097 frames and 2 tokens exceed the limits of 4096 frames and 1024"):
            fn(torch.zeros(1, 4097, 2).to(device))
        with pytest.raises(ValueError, match="forward_sum: utterance 0: 1030 frames and 1025 tokens exceed the limits"):
            fn(torch.zeros(1, 1030, 1025).to(device))
        with pytest.raises(TypeError, match="forward_sum: expected a float32"):
            fn(x.double())
        with pytest.raises(TypeError, match="forward_sum: expected a float32"):
            fn([[0.0]])
        for bad in (torch.zeros(4).to(device), torch.zeros(1, 2, 3, 3).to(device)):
            with pytest.raises(ValueError, match=r"forward_sum: expected \(B, T, N\) or \(T, N\)"):
                fn(bad)
        with pytest.raises(ValueError, match="forward_sum: t_1 lengths for a batch of 2"):
            fn(x, [6], [4, 4])
    # a longer buffer holding shorter utterances is accepted, whatever the buffer's own size
    g, d, lz = alignment.alignment_posterior(torch.zeros(1, 4100, 3).to(device), [5], [2])
    assert g.shape == (1, 4100, 3) and d.shape == (1, 3) and abs(float(lz[0]) - math.log(4.0)) < 1e-6
    assert abs(float(d[0, :2].sum()) - 5.0) < 1e-5 and float(d[0, 2]) == 0.0 and not g[0, 5:].any() and not g[0, :, 2:].any()
