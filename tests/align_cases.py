"""The cases and assertions the CPU file (csrc/align.hip on the host stand-in) and the GPU file (the MI355X) of the alignment
tests share: every check takes a ``device`` and runs tacotron2_amd.native / tacotron2_amd.alignment on tensors of that device."""
import functools

import numpy as np
import torch

import align_ref as ar
from tacotron2_amd import alignment, native

W = 256                                                                     # lanes of the workgroup (checked against the library)
POISON, IPOISON, BPOISON = -777.0, -77, 0xEE
SHAPES = [(1, 1), (2, 1), (2, 2), (9, 1), (7, 7), (65, 64), (130, 63), (130, 65), (W + 1, W - 1), (W + 3, W), (W + 40, W + 1),
          (1030, 1024), (4096, 5)]
KINDS = ("log_softmax", "mixed_sign")


@functools.lru_cache(maxsize=None)
def matrix(T, N, kind, seed=0):
    """(scores, the float32 restatement's result, the float64 one's) of one case, computed once."""
    g = np.random.RandomState(1000 * seed + 7 * T + N)
    x = ar.log_softmax_rows(g, T, N) if kind == "log_softmax" else ar.mixed_sign(g, T, N)
    x.setflags(write=False)
    return x, ar.align32(x), ar.align64(x)


def _round4(n):
    return (n + 3) // 4 * 4


def run(mats, device, offset=0, pad=3):
    """The native launch on poisoned outputs and a poisoned workspace for a ragged batch of (T, N) float32 matrices, without and
    with the path.  The batch is a view into a wider buffer that starts ``offset`` floats into its rows and holds 1e30 wherever
    no utterance is.  -> (durations, score, path) as numpy, after checking that the two calls agree bit for bit, the invariants
    of every utterance, and that nothing was written outside an utterance's own region of any buffer."""
    B = len(mats)
    tl, nl = [m.shape[0] for m in mats], [m.shape[1] for m in mats]
    Tm, Nm = max(tl), max(nl)
    buf = torch.full((B, Tm + 1, offset + Nm + pad), 1e30)
    for b, m in enumerate(mats):
        buf[b, :tl[b], offset:offset + nl[b]] = torch.from_numpy(np.array(m))
    x = buf.to(device)[:, :Tm, offset:offset + Nm]
    t_dev, n_dev = (torch.tensor(v, dtype=torch.int32).to(device) for v in (tl, nl))
    nbytes = native.align_workspace(B, Tm, Nm)
    ldw = _round4(Nm)
    slab_bytes = (B * Tm * ldw + 7) // 8 * 8
    assert nbytes == slab_bytes + 16 * B
    got = []
    for with_path in (False, True):
        dur = torch.full((B, Nm), IPOISON, dtype=torch.int32, device=device)
        score = torch.full((B,), POISON, device=device)
        path = torch.full((B, Tm), IPOISON, dtype=torch.int32, device=device) if with_path else None
        ws = torch.full((nbytes,), BPOISON, dtype=torch.uint8, device=device)
        native.monotonic_align(x, t_dev, n_dev, dur, score, path, ws)
        got.append((dur.cpu().numpy(), score.cpu().numpy(), None if path is None else path.cpu().numpy()))
        slab = ws.cpu().numpy()[:B * Tm * ldw].reshape(B, Tm, ldw)
        for b in range(B):                                                  # rows 1 .. T-1, columns below N (rounded up to 4 where
            cols = nl[b] if Nm <= W else _round4(nl[b])                     # a lane stores its four columns at once)
            own = slab[b, 1:tl[b], :cols]
            assert (own <= 1).all(), b
            assert (slab[b, 0] == BPOISON).all() and (slab[b, tl[b]:] == BPOISON).all() and (slab[b, :, cols:] == BPOISON).all(), b
        assert (ws.cpu().numpy()[B * Tm * ldw:slab_bytes] == BPOISON).all()
    (d0, s0, _), (dur, score, path) = got
    assert np.array_equal(d0, dur) and np.array_equal(s0.view(np.int32), score.view(np.int32))
    for b in range(B):
        T, N = tl[b], nl[b]
        assert dur[b].sum() == T and (dur[b, :N] >= 1).all() and not dur[b, N:].any(), b
        assert ar.is_admissible(path[b, :T], T, N) and (path[b, T:] == -1).all(), b
        assert np.array_equal(np.bincount(path[b, :T], minlength=Nm), dur[b]), b
    return dur, score, path


def check_matrix(x, ref32, ref64, dur, score, path):
    """The kernel's result for one utterance against the two restatements: bit for bit the float32 one's, and within
    (T + 2) u S of the float64 optimum.  -> the worst fraction of the bound."""
    T, N = x.shape
    s32, d32, p32 = ref32
    assert np.float32(score).view(np.int32) == np.float32(s32).view(np.int32), (T, N, float(score), float(s32))
    assert np.array_equal(dur[:N], d32) and np.array_equal(path[:T], p32), (T, N)
    returned, S = ar.path_score(x, path[:T])
    tol = ar.bound(T, S)
    e_opt, e_sum = abs(returned - float(ref64[0])), abs(float(score) - returned)
    assert e_opt <= tol and e_sum <= tol, (T, N, e_opt, e_sum, tol)
    return max(e_opt, e_sum) / tol if tol > 0 else 0.0


def check_shape(T, N, kind, device):
    x, ref32, ref64 = matrix(T, N, kind)
    dur, score, path = run([x], device, offset=(T + N) % 3)
    frac = check_matrix(x, ref32, ref64, dur[0], score[0], path[0])
    print("FIGURE %s (%d, %d): score %.6f, float64 optimum %.6f, error / bound %.4f" % (kind, T, N, float(score[0]),
                                                                                         float(ref64[0]), frac))
    assert native.align_limits() == (W, alignment.MAX_FRAMES, alignment.MAX_TOKENS)


def ties(device):
    """Exact ties are decided by the tie rule alone: staying wins."""
    for T, N in ((1, 1), (5, 5), (9, 4), (W + 9, W + 2), (300, 7)):
        dur, score, _ = run([np.zeros((T, N), np.float32)], device)
        assert dur[0].tolist() == [1] * (N - 1) + [T - N + 1] and score[0] == 0.0, (T, N)
    g = np.random.RandomState(3)
    # two identical columns, and a matrix equal along time: the restatement's result, exactly
    x = ar.mixed_sign(g, 40, 9)
    x[:, 5] = x[:, 4]
    y = np.repeat(ar.mixed_sign(g, 1, 70), 200, axis=0)
    z = np.repeat(ar.log_softmax_rows(g, 1, W + 30), W + 77, axis=0)
    for m in (x, y, z):
        dur, score, path = run([m], device)
        check_matrix(m, ar.align32(m), ar.align64(m), dur[0], score[0], path[0])


def planted(device):
    """A random admissible path raised by 3 over noise in [-1, 0]: every other path loses at least 2 per cell it leaves."""
    g = np.random.RandomState(11)
    for T, N in ((40, 40), (300, 97), (600, 300)):
        want = ar.random_path(g, T, N)
        x = -g.rand(T, N).astype(np.float32)
        x[np.arange(T), want] += np.float32(3.0)
        dur, _, path = run([x], device)
        assert np.array_equal(path[0], want) and np.array_equal(dur[0], np.bincount(want, minlength=N)), (T, N)


def ragged_mats():
    g = np.random.RandomState(5)
    return [ar.log_softmax_rows(g, 130, 65), ar.mixed_sign(g, 9, 1), ar.mixed_sign(g, 64, 64), ar.log_softmax_rows(g, 200, 31),
            np.zeros((77, 12), np.float32), ar.mixed_sign(g, 1, 1)]


def ragged_equals_alone(mats, device):
    """A ragged batch gives each utterance the bits it gives alone (at another buffer stride), and two calls agree."""
    one = run(mats, device, offset=1)
    two = run(mats, device, offset=1)
    for a, b in zip(one, two):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for b, m in enumerate(mats):
        T, N = m.shape
        dur, score, path = run([m], device, offset=b % 3, pad=b)
        assert np.array_equal(one[0][b, :N], dur[0]) and np.array_equal(one[2][b, :T], path[0]), b
        assert one[1].view(np.int32)[b] == score.view(np.int32)[0], b
        check_matrix(m, ar.align32(m), ar.align64(m), dur[0], score[0], path[0])


def module_equals_native(mats, device):
    """alignment.monotonic_align on the padded batch: the bits of the native calls, with and without the path; a (T, N) matrix is
    a batch of one; a longer buffer holding shorter utterances is accepted."""
    dur, score, path = run(mats, device)
    tl, nl = [m.shape[0] for m in mats], [m.shape[1] for m in mats]
    x = torch.zeros(len(mats), max(tl) + 2, max(nl) + 3)
    for b, m in enumerate(mats):
        x[b, :tl[b], :nl[b]] = torch.from_numpy(m)
    x = x.to(device).requires_grad_(True)
    a = alignment.monotonic_align(x, tl, nl)
    c = alignment.monotonic_align(x, torch.tensor(tl), torch.tensor(nl), return_path=True)
    assert len(a) == 2 and len(c) == 3 and all(t.grad_fn is None and not t.requires_grad for t in c)
    assert c[0].shape == (len(mats), max(nl) + 3) and c[2].shape == (len(mats), max(tl) + 2) and c[0].dtype == torch.int32
    assert np.array_equal(c[0].cpu().numpy()[:, :max(nl)], dur) and not c[0].cpu().numpy()[:, max(nl):].any()
    assert np.array_equal(c[2].cpu().numpy()[:, :max(tl)], path) and (c[2].cpu().numpy()[:, max(tl):] == -1).all()
    assert np.array_equal(c[1].cpu().numpy().view(np.int32), score.view(np.int32))
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    single = alignment.monotonic_align(x.detach()[0, :tl[0], :nl[0]])
    assert single[0].shape == (1, nl[0]) and np.array_equal(single[0].cpu().numpy()[0], dur[0, :nl[0]])


def many_short(device):
    """300 utterances: more workgroups than compute units."""
    g = np.random.RandomState(21)
    mats = []
    for _ in range(300):
        T = int(g.randint(1, 12))
        mats.append(ar.mixed_sign(g, T, int(g.randint(1, T + 1))))
    dur, score, path = run(mats, device, offset=2)
    worst = 0.0
    for b, m in enumerate(mats):
        worst = max(worst, check_matrix(m, ar.align32(m), ar.align64(m), dur[b], score[b], path[b]))
    print("FIGURE 300 utterances of 1 to 11 frames: worst error / bound %.4f" % worst)


def attention_case(device):
    """alignment.attention_durations on a softmax of planted scores that holds exact zeros: the planted path comes back, the
    clamp at eps is what keeps the zeros finite."""
    g = np.random.RandomState(13)
    To, Ti = [50, 33], [20, 33]
    A = torch.zeros(2, 50, 33)
    want = []
    for b in range(2):
        p = ar.random_path(g, To[b], Ti[b])
        z = g.randn(To[b], Ti[b])
        z[np.arange(To[b]), p] += 8.0                                       # on the path more than half of a row's mass
        z[g.rand(To[b], Ti[b]) < 0.3] = -200.0                              # exp(-200) is 0 in float32
        z[np.arange(To[b]), p] = np.maximum(z[np.arange(To[b]), p], 6.0)
        A[b, :To[b], :Ti[b]] = torch.softmax(torch.from_numpy(z).float(), dim=1)
        want.append(p)
        assert (A[b, :To[b], :Ti[b]] == 0).any() and (A[b, np.arange(To[b]), p] > 0.5).all()
    A = A.to(device)
    dur, score, path = alignment.attention_durations(A, Ti, To, return_path=True)
    again = alignment.monotonic_align(torch.log(A.clamp_min(1e-8)), To, Ti, return_path=True)
    for x, y in zip((dur, score, path), again):
        assert torch.equal(x, y)
    assert torch.isfinite(score).all() and len(alignment.attention_durations(A, Ti, To)) == 2
    for b in range(2):
        assert np.array_equal(path[b, :To[b]].cpu().numpy(), want[b]) and (path[b, To[b]:] == -1).all()
        assert np.array_equal(dur[b].cpu().numpy(), np.bincount(want[b], minlength=33))
    m = alignment.alignment_metrics(A, path, Ti, To)
    assert (m["off_path"] == 0).all() and (m["backward_steps"] == 0).all() and (m["path_mass"] > 0.5).all()
    assert np.array_equal(m["focus"], m["path_mass"]) and m["max_duration"].tolist() == [np.bincount(w).max() for w in want]


def refusals(device):
    """The refusals of section 18.1, each by its message."""
    import pytest
    x = torch.zeros(2, 6, 4).to(device)
    with pytest.raises(ValueError, match="utterance 1 has 4 tokens and only 3 frames"):
        alignment.monotonic_align(x, [6, 3], [4, 4])
    with pytest.raises(ValueError, match=r"utterance 0: 0 frames and 1 tokens do not lie in \[1, 6\] and \[1, 4\]"):
        alignment.monotonic_align(x, [0, 3], [1, 1])
    with pytest.raises(ValueError, match="utterance 1: 3 frames and 0 tokens do not lie"):
        alignment.monotonic_align(x, [6, 3], [4, 0])
    with pytest.raises(ValueError, match="utterance 1: 7 frames and 1 tokens do not lie"):
        alignment.monotonic_align(x, [6, 7], [4, 1])
    with pytest.raises(ValueError, match="utterance 0 has 4 tokens and only 3 frames"):
        alignment.monotonic_align(torch.zeros(3, 4).to(device))
    with pytest.raises(ValueError, match="utterance 0: 4097 frames and 2 tokens exceed the limits of 4096 frames and 1024 tokens"):
        alignment.monotonic_align(torch.zeros(1, 4097, 2).to(device))
    with pytest.raises(ValueError, match="utterance 0: 1030 frames and 1025 tokens exceed the limits"):
        alignment.monotonic_align(torch.zeros(1, 1030, 1025).to(device))
    with pytest.raises(TypeError, match="float32"):
        alignment.monotonic_align(x.double())
    with pytest.raises(TypeError, match="float32"):
        alignment.monotonic_align([[0.0]])
    for bad in (torch.zeros(4).to(device), torch.zeros(1, 2, 3, 3).to(device)):
        with pytest.raises(ValueError, match=r"\(B, T, N\) or \(T, N\)"):
            alignment.monotonic_align(bad)
    with pytest.raises(ValueError, match="lengths for a batch of 2"):
        alignment.monotonic_align(x, [6], [4, 4])
    # a longer buffer holding shorter utterances is accepted, whatever the buffer's own size
    dur, _ = alignment.monotonic_align(torch.zeros(1, 4100, 3).to(device), [5], [2])
    assert dur.cpu().tolist() == [[1, 4, 0]]
