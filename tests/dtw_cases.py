"""The cases and assertions the CPU file (kernel source on the host stand-in) and the GPU file (the MI355X) of the DTW tests
share: every check takes a ``device`` and runs tacotron2_amd.native / tacotron2_amd.audio on tensors of that device."""
import numpy as np
import torch

import dtw_ref as dr
from tacotron2_amd import audio, native

POISON_F, POISON_I, POISON_B = -777.0, -777, 0xEE
KS = (1, 13, 32)


def length_pairs():
    W = native.dtw_width()
    return [(1, 1), (1, 7), (7, 1), (2, 2), (63, 65), (W - 1, W + 1), (W, W), (W + 1, 40), (2 * W + 1, 70)]


def run(pairs, device, slab_check=True):
    """The native launches on poisoned outputs for a batch of (a, b) float32 numpy pairs of one K: the cost-only call, the call
    with the path, the backtrack.  Padding rows hold 1e30.  -> (cost, steps, path) as numpy, after checking that the two calls
    agree bit for bit, that every output element was written and that the slab was written inside each pair's cells only."""
    B, K = len(pairs), pairs[0][0].shape[1]
    la, lb = [p[0].shape[0] for p in pairs], [p[1].shape[0] for p in pairs]
    Ta, Tb = max(la), max(lb)
    x, y = torch.full((B, Ta, K), 1e30), torch.full((B, Tb, K), 1e30)
    for p, (a, b) in enumerate(pairs):
        x[p, :la[p]] = torch.from_numpy(a)
        y[p, :lb[p]] = torch.from_numpy(b)
    x, y = x.to(device), y.to(device)
    na, nb = torch.tensor(la, dtype=torch.int32).to(device), torch.tensor(lb, dtype=torch.int32).to(device)

    def outputs():
        return (torch.full((B,), POISON_F, device=device), torch.full((B,), POISON_I, dtype=torch.int32, device=device))
    cost, steps = outputs()
    native.dtw(x, y, na, nb, cost, steps)
    cost2, steps2 = outputs()
    slab = torch.full((B, Ta, Tb), POISON_B, dtype=torch.uint8, device=device)
    path = torch.full((B, Ta + Tb - 1, 2), POISON_I, dtype=torch.int32, device=device)
    native.dtw(x, y, na, nb, cost2, steps2, slab)
    native.dtw_backtrack(slab, na, nb, steps2, Ta, Tb, path)
    cost, steps, cost2, steps2, slab, path = (t.cpu() for t in (cost, steps, cost2, steps2, slab, path))
    assert torch.equal(cost.view(torch.int32), cost2.view(torch.int32)) and torch.equal(steps, steps2)
    assert not (steps == POISON_I).any() and not (cost == POISON_F).any() and not (path == POISON_I).any()
    if slab_check:
        for p in range(B):
            inside = slab[p, :la[p], :lb[p]]
            assert int(inside.max()) <= 2
            outside = slab[p].clone()
            outside[:la[p], :lb[p]] = POISON_B
            assert (outside == POISON_B).all()
    return cost.numpy(), steps.numpy(), path.numpy()


def check_pair(a, b, cost, steps, path, identity=None):
    """The assertions of one pair: optimum within the bound, a warping path of ``steps`` cells whose float64 cost is within the
    bound, -1 beyond it; path identity with the restatement when ``identity`` (or, when None, where the restatement's optimum is
    unique by margin).  -> whether identity was demanded."""
    n_a, n_b, K = a.shape[0], b.shape[0], a.shape[1]
    opt, ref_steps, ref_path = dr.dtw(a, b)
    tol = dr.bound(n_a, n_b, K)
    rel = abs(float(cost) - opt) / opt if opt > 0 else abs(float(cost))
    print("FIGURE (%d, %d) K=%d: cost %.9g optimum %.9g relative %.3e bound %.3e steps %d"
          % (n_a, n_b, K, float(cost), opt, rel, tol, int(steps)))
    assert abs(float(cost) - opt) <= tol * opt
    own = [tuple(int(v) for v in ij) for ij in path[:int(steps)]]
    assert (path[int(steps):] == -1).all() and max(n_a, n_b) <= int(steps) <= n_a + n_b - 1
    assert dr.is_warping_path(own, n_a, n_b)
    assert abs(dr.path_cost(a, b, own) - opt) <= tol * opt
    if identity is None:
        identity = dr.unique_by_margin(a, b)
    if identity:
        assert own == ref_path and int(steps) == ref_steps
    return identity


def check_lengths(n_a, n_b, K, device, seed=0):
    a, b = dr.sequences(n_a, n_b, K, 1000 * seed + 7 * n_a + n_b + K)
    cost, steps, path = run([(a, b)], device)
    check_pair(a, b, cost[0], steps[0], path[0])
    return cost[0], steps[0], path[0]


def margin_seeds(device, tried=24):
    """Random pairs with n_a, n_b <= 16: where the restatement's optimum is unique by margin the path must be the restatement's.
    -> the number of seeds that qualified."""
    qualified = 0
    for seed in range(tried):
        g = np.random.RandomState(500 + seed)
        n_a, n_b, K = int(g.randint(2, 17)), int(g.randint(2, 17)), (1, 13, 32)[seed % 3]
        a, b = g.randn(n_a, K).astype(np.float32), g.randn(n_b, K).astype(np.float32)
        if not dr.unique_by_margin(a, b):
            continue
        qualified += 1
        cost, steps, path = run([(a, b)], device)
        assert check_pair(a, b, cost[0], steps[0], path[0], identity=True)
    return qualified


def tie_cases(device):
    """Exact ties, decided by the tie rule alone: each must equal the restatement exactly."""
    g = np.random.RandomState(3)
    for K in KS:
        for n in (1, 5, 40):
            a = g.randn(n, K).astype(np.float32)
            cost, steps, path = run([(a, a.copy())], device)
            assert cost[0] == 0.0 and steps[0] == n
            assert [tuple(v) for v in path[0, :n]] == [(i, i) for i in range(n)] and (path[0, n:] == -1).all()
        zeros = [(np.zeros((n_a, K), np.float32), np.zeros((n_b, K), np.float32)) for n_a, n_b in ((3, 7), (9, 2), (1, 6), (300, 2))]
        single = [(g.randn(1, K).astype(np.float32), g.randn(6, K).astype(np.float32)),
                  (g.randn(6, K).astype(np.float32), g.randn(1, K).astype(np.float32))]
        for a, b in zeros + single:
            n_a, n_b = a.shape[0], b.shape[0]
            cost, steps, path = run([(a, b)], device)
            opt, ref_steps, ref_path = dr.dtw(a, b)
            assert steps[0] == ref_steps == max(n_a, n_b)
            assert [tuple(int(v) for v in ij) for ij in path[0, :ref_steps]] == ref_path
            assert abs(float(cost[0]) - opt) <= dr.bound(n_a, n_b, K) * opt


def ragged_pairs(K=13):
    shapes = [(9, 11), (1, 4), (30, 17), (5, 5), (2, 23)]
    return [dr.sequences(n_a, n_b, K, 40 + i) for i, (n_a, n_b) in enumerate(shapes)]


def ragged_equals_alone(pairs, device):
    """A ragged batch gives each pair the bits it gives alone, and two calls give equal bits."""
    cost, steps, path = run(pairs, device)
    again = run(pairs, device)
    assert np.array_equal(cost.view(np.int32), again[0].view(np.int32)) and np.array_equal(steps, again[1])
    assert np.array_equal(path, again[2])
    for p, (a, b) in enumerate(pairs):
        c1, s1, p1 = run([(a, b)], device)
        assert c1.view(np.int32)[0] == cost.view(np.int32)[p] and s1[0] == steps[p]
        assert np.array_equal(p1[0, :s1[0]], path[p, :steps[p]]) and (path[p, steps[p]:] == -1).all()
        check_pair(a, b, cost[p], steps[p], path[p])


def module_equals_native(pairs, device):
    """audio.dtw on the padded batch: the bits of the native calls, with and without the path."""
    cost, steps, path = run(pairs, device)
    la, lb = [p[0].shape[0] for p in pairs], [p[1].shape[0] for p in pairs]
    K = pairs[0][0].shape[1]
    x, y = torch.zeros(len(pairs), max(la) + 2, K), torch.zeros(len(pairs), max(lb) + 3, K)
    for p, (a, b) in enumerate(pairs):
        x[p, :la[p]] = torch.from_numpy(a)
        y[p, :lb[p]] = torch.from_numpy(b)
    c, s = audio.dtw(x.to(device), y.to(device), la, lb)
    c2, s2, pth = audio.dtw(x.to(device), y.to(device), la, lb, return_path=True)
    assert c.dtype == torch.float32 and s.dtype == torch.int32 and pth.dtype == torch.int32
    assert pth.shape == (len(pairs), max(la) + max(lb) - 1, 2)
    assert np.array_equal(c.cpu().numpy().view(np.int32), cost.view(np.int32)) and np.array_equal(s.cpu().numpy(), steps)
    assert torch.equal(c.cpu(), c2.cpu()) and torch.equal(s.cpu(), s2.cpu()) and np.array_equal(pth.cpu().numpy(), path)


def stretched_mels(n_mel=80, T=120, seed=5, ratio=1.13):
    """A (1, n_mel, T) log-mel-like array and a time-stretched noisy copy of it."""
    g = np.random.RandomState(seed)
    t = np.arange(T + 8)
    mel = -5.0 + 1.5 * np.cumsum(g.randn(n_mel, T + 8), axis=1) / np.sqrt(t + 1.0) + 0.8 * np.sin(np.arange(n_mel)[:, None] / 7.0)
    Tb = int(round(T * ratio))
    src = np.linspace(0, T - 1, Tb)
    other = np.stack([np.interp(src, np.arange(T), mel[m, :T]) for m in range(n_mel)]) + 0.05 * g.randn(n_mel, Tb)
    return mel[None, :, :T].astype(np.float32), other[None].astype(np.float32)


def mcd_end_to_end(device, cep_err):
    """MelCepstralDistortion on a (80, 120) mel against a time-stretched noisy copy: the restatement's MCD (float64 cepstra,
    float64 DTW) within the derived bound plus the cepstral error.  ``cep_err``: the bound on |c32 - c64| per frame (2-norm)
    relative to nothing, i.e. absolute; every local cost moves by at most twice it."""
    ma, mb = stretched_mels()
    mod = audio.MelCepstralDistortion(13)
    a, b = torch.from_numpy(ma).to(device).requires_grad_(True), torch.from_numpy(mb).to(device)
    got = mod(a, b)
    assert got.shape == (1,) and got.grad_fn is None and not got.requires_grad
    last = mod.last
    assert sorted(last) == ["cost", "len_a", "len_b", "steps"] and last["len_a"] == [120] and last["len_b"] == [mb.shape[2]]
    assert last["cost"].grad_fn is None and last["steps"].dtype == torch.int32
    ca, cb = dr.cepstrum(ma)[0], dr.cepstrum(mb)[0]
    opt, ref_steps, _ = dr.dtw(ca, cb)
    steps = int(last["steps"].cpu()[0])
    n_a, n_b = 120, mb.shape[2]
    # cost: every local cost of either path moves by at most 2 cep_err, over at most n_a + n_b - 1 cells; then the bound
    slack = 2.0 * cep_err * (n_a + n_b - 1) + dr.bound(n_a, n_b, 13) * opt
    cost = float(last["cost"].cpu()[0])
    print("FIGURE MCD end to end: cost %.9g restatement %.9g, allowed %.3e; MCD %.6f dB, restatement %.6f dB (steps %d / %d)"
          % (cost, opt, slack, float(got.cpu()[0]), dr.mcd(opt, ref_steps), steps, ref_steps))
    assert abs(cost - opt) <= slack
    assert max(n_a, n_b) <= steps <= n_a + n_b - 1
    want = dr.mcd(cost, steps)
    assert abs(float(got.cpu()[0]) - want) <= 4 * 2.0 ** -24 * want
    if steps == ref_steps:
        assert abs(float(got.cpu()[0]) - dr.mcd(opt, ref_steps)) <= dr.MCD_DB * slack / steps + 4 * 2.0 ** -24 * want
    return float(got.cpu()[0])


def cepstrum_errors(device, n_mel=80, T=257, lengths=(257, 100, 1), Ks=KS):
    """mel_cepstrum against the float64 restatement: -> {K: (kernel max abs error, float32 torch.matmul max abs error)} and checks
    the zero rows beyond the lengths on a poisoned output."""
    g = np.random.RandomState(11)
    mel = (-5.0 + 2.0 * g.randn(len(lengths), n_mel, T)).astype(np.float32)
    out = {}
    for K in Ks:
        want = dr.cepstrum(mel, K, lengths)
        dev_mel = torch.from_numpy(mel).to(device)
        got = audio.mel_cepstrum(dev_mel, list(lengths), K)
        assert got.shape == (len(lengths), T, K) and got.dtype == torch.float32
        for b, n in enumerate(lengths):
            assert not got[b, n:].cpu().any()
        basis = torch.from_numpy(audio.cepstral_basis(n_mel, K)).to(device)
        mm = torch.matmul(dev_mel.transpose(1, 2), basis.t()).cpu().double().numpy()
        for b, n in enumerate(lengths):
            mm[b, n:] = 0.0
        e_k = np.abs(got.cpu().double().numpy() - want).max()
        e_t = np.abs(mm - want).max()
        out[K] = (float(e_k), float(e_t))
        full = audio.mel_cepstrum(dev_mel, None, K)
        assert torch.equal(full[0], got[0])                     # the full utterance of the ragged batch: the same bits
        alone = audio.mel_cepstrum(dev_mel[1:2, :, :lengths[1]].contiguous(), None, K)
        assert torch.equal(alone[0], got[1, :lengths[1]])
    return out
