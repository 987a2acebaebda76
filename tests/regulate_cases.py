"""The cases of the length regulator that tests/test_regulate_cpu.py runs on the host stand-in and
tests/test_zz27_regulate_gpu.py on the device: the same functions, given the device.  The native entries are called on outputs
poisoned with NaN / 0x7f bytes; the references are tests/regulate_ref.py's, computed once per utterance and shared."""
import functools

import numpy as np
import torch

import regulate_ref as rr

# (N, S, C, heavy): tokens, frames, channels; heavy gives one token all but a few of the frames
SHAPES = [(1, 1, 1, False), (1, 0, 1, False), (2, 2, 3, False), (5, 9, 4, False), (7, 7, 5, False), (63, 130, 32, False),
          (64, 65, 64, False), (65, 130, 80, False), (255, 511, 257, False), (256, 512, 257, False), (257, 513, 257, False),
          (1024, 1030, 512, False), (5, 4096, 80, True), (1, 4096, 1, False)]
PATTERNS = ("ones", "zeros", "allzero")
WEIGHTS = {"ones": "frac", "zeros": "flags", "allzero": None}
MAX_ULPS = 0                            # of the quotient and of dv from the float32 restatement: the build divides correctly rounded
                                        # (section 21.4: 0 on every case measured, so equality is asserted)
RAGGED_N = (0, 1, 5, 64, 65, 130)


def _t(a):
    return torch.from_numpy(np.array(a))                                    # the cached arrays are read-only


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def durations(N, S, pattern, heavy=False, seed=0):
    """N durations that sum to S (0 for ``allzero``): all >= 1, or with zeros at the start, at the end and two in a row in the
    middle.  None where the pattern does not fit."""
    g = np.random.RandomState(17 * N + S + 1000 * seed)
    d = np.zeros(N, dtype=np.int64)
    if pattern == "allzero":
        return d
    zero = set() if pattern == "ones" else {0, N - 1, N // 2, N // 2 + 1} & set(range(N))
    live = [n for n in range(N) if n not in zero]
    if not live or S < len(live) or (pattern == "zeros" and not zero):
        return None
    d[live] = 1
    extra = S - len(live)
    if heavy:
        mid = live[len(live) // 2]
        d[mid] += max(extra - 5, 0)
        extra -= max(extra - 5, 0)
    d[live] += g.multinomial(extra, np.full(len(live), 1.0 / len(live)))
    assert d.sum() == S
    return d


def t_variants(d):
    """S, beyond S, a cut exactly at a segment's end, a cut one frame into a segment, 0."""
    S, e = int(d.sum()), np.cumsum(d)
    out = [S, S + 3]
    inner = [int(v) for v in e if 0 < v < S]
    if inner:
        k = inner[len(inner) // 2]
        out += [k] + ([k + 1] if k + 1 < S else [])
    return out + [0]


@functools.lru_cache(maxsize=None)
def utterance(d, C, T, wkind, seed=0):
    """One utterance's operands and both restatements; ``d`` is a tuple, ``T`` the buffer's frame count."""
    N = len(d)
    g = np.random.RandomState((seed * 1000003 + N * 7919 + (sum(d) % 65521) * 31 + C + 101 * T) % (2 ** 32))
    path, Tb = rr.path_of(d, N, T)
    x, dy, v, gm = (g.randn(r, C).astype(np.float32) for r in (N, T, T, N))
    flat = x.reshape(-1)
    for i, special in enumerate((-0.0, np.inf, -np.inf, np.nan, 1e-41)):     # a copy keeps every bit
        if N * C > 2 * i:
            flat[(2 * i) % (N * C)] = np.float32(special)
    w = None
    if wkind == "flags":
        w = (g.rand(T) < 0.6).astype(np.float32)
    elif wkind == "frac":
        w = g.rand(T).astype(np.float32)
    owners = [n for n in range(N) if (path == n).any()]
    if w is not None and owners:                                             # one token whose frames all weigh 0
        w[path == owners[len(owners) // 2]] = 0.0
    w1 = np.ones(T, np.float32) if w is None else w
    p64, p32 = rr.pool64(v, w1, path, N), rr.pool32(v, w1, path, N)
    dx64, mag, cnt = rr.segsum64(dy, path, N)
    u = dict(d=np.array(d, dtype=np.int64), N=N, C=C, T=T, Tb=Tb, path=path, x=x, dy=dy, v=v, g=gm, w=w, y=rr.expand(x, path),
             dx32=rr.segsum32(dy, path, N), dx64=dx64, dx_mag=mag, cnt=cnt, p64=p64, p32=p32,
             dv32=rr.pool_bwd(gm, p32["den"], w1, path, np.float32), dv64=rr.pool_bwd(gm, p64["den"], w1, path, np.float64))
    for a in u.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return u


def run(utts, device, T, offset=0, pad=0, dur_dtype=torch.int32, lengths=True):
    """The five native entries on a ragged batch of ``utterance`` dicts at the frame count ``T``: x is a slice of a flat buffer
    that starts ``offset`` floats in, the token buffers are ``pad`` tokens wider than the longest utterance needs and
    hold junk (1e30, and large and negative durations) wherever no utterance is.  -> the outputs as numpy."""
    from tacotron2_amd import native as nv
    B, C = len(utts), utts[0]["C"]
    N = max(max(u["N"] for u in utts), 1)
    N = max(N, min(N + pad, 1024))                                          # the limit of the entries
    d = torch.full((B, N), -2 ** 31 + 5, dtype=dur_dtype)
    d[:, N // 2:] = 2 ** 31 - 7
    flat = torch.full((offset + B * N * C + 4,), 1e30)
    x = flat[offset:offset + B * N * C].view(B, N, C)
    dy, v, w, g = torch.full((B, max(T, 1), C), 1e30), torch.full((B, max(T, 1), C), 1e30), torch.full((B, max(T, 1)), 1e30), torch.full((B, N, C), 1e30)
    for b, u in enumerate(utts):
        assert u["T"] == T and u["C"] == C
        n = u["N"]
        d[b, :n], x[b, :n], g[b, :n] = _t(u["d"]).to(dur_dtype), _t(u["x"]), _t(u["g"])
        if T:
            dy[b], v[b] = _t(u["dy"]), _t(u["v"])
            w[b] = 1.0 if u["w"] is None else _t(u["w"])
    weighted = any(u["w"] is not None for u in utts)
    if not lengths:
        assert all(u["N"] == N for u in utts)
    n_dev = torch.tensor([u["N"] for u in utts], dtype=torch.int32).to(device) if lengths else None
    flat = flat.to(device)
    x = flat[offset:offset + B * N * C].view(B, N, C)
    d, dy, v, w, g = (t.to(device) for t in (d, dy, v, w, g))
    ipoison = lambda *s: torch.full(s, 0x7f7f7f7f, dtype=torch.int32).to(device)          # noqa: E731
    fpoison = lambda *s: torch.full(s, float("nan")).to(device)                            # noqa: E731
    path, t_lengths, ends = ipoison(B, T), ipoison(B), ipoison(B, N)
    totals = torch.full((B,), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64).to(device)
    nv.durations_to_path(d, n_dev, T, path, t_lengths, ends, totals)
    out = dict(path=path, t_lengths=t_lengths, ends=ends, totals=totals)
    if T:
        y, dx, mean, den, num, dv = fpoison(B, T, C), fpoison(B, N, C), fpoison(B, N, C), fpoison(B, N), fpoison(B, N, C), fpoison(B, T, C)
        nv.length_regulate(x, path, y)
        nv.length_regulate_backward(dy, ends, dx)
        nv.token_average(v, w if weighted else None, ends, mean, den, num)
        nv.token_average_backward(g, den, w if weighted else None, path, dv)
        out.update(y=y, dx=dx, m=mean, den=den, num=num, dv=dv)
    return {k: t.cpu().numpy() for k, t in out.items()}


def check(u, out, b=0, label=""):
    """Utterance ``b`` of ``out`` against both restatements.  -> the worst ulps of the quotient and of dv, and the worst
    fractions of the three float64 allowances."""
    N, T, Tb, C = u["N"], u["T"], u["Tb"], u["C"]
    assert out["t_lengths"][b] == Tb and out["totals"][b] == int(u["d"].sum()), (label, b)
    assert np.array_equal(out["path"][b], u["path"]), (label, b)
    assert np.array_equal(out["ends"][b, :N], np.minimum(np.cumsum(u["d"]), T)) and (out["ends"][b, N:] == Tb).all(), (label, b)
    if not T:
        return 0, 0, 0.0, 0.0, 0.0
    assert np.array_equal(bits(out["y"][b]), bits(u["y"])), (label, b, "y")
    for name in ("dx", "num", "m"):                                         # exact +0 at and beyond N_b
        assert not bits(out[name][b, N:]).any(), (label, b, name)
    assert not bits(out["den"][b, N:]).any() and not bits(out["dv"][b, Tb:]).any(), (label, b)
    assert np.array_equal(bits(out["dx"][b, :N]), bits(u["dx32"])), (label, b, "dx")
    allow = rr.gamma(u["cnt"] - 1)[:, None] * u["dx_mag"]
    err = np.abs(out["dx"][b, :N].astype(np.float64) - u["dx64"])
    assert (err <= allow).all(), (label, b, "dx against float64")
    f_dx = float((err / np.where(allow > 0, allow, 1.0)).max()) if N else 0.0
    assert np.array_equal(bits(out["num"][b, :N]), bits(u["p32"]["num"])), (label, b, "num")
    assert np.array_equal(bits(out["den"][b, :N]), bits(u["p32"]["den"])), (label, b, "den")
    ulp_m = int(rr.ulps(out["m"][b, :N], u["p32"]["m"]).max()) if N else 0
    ulp_dv = int(rr.ulps(out["dv"][b], u["dv32"]).max())
    assert ulp_m <= MAX_ULPS and ulp_dv <= MAX_ULPS, (label, b, ulp_m, ulp_dv)
    allow = rr.pool_allowed(u["p64"])
    err = np.abs(out["m"][b, :N].astype(np.float64) - u["p64"]["m"])
    assert (err <= allow).all(), (label, b, "m against float64")
    f_m = float((err / np.where(allow > 0, allow, 1.0)).max()) if N else 0.0
    # dv = w (g / den): den within gamma_{m-1} of the float64 one, one division, one product, doubled for the second-order terms
    per_frame = np.where(u["path"] >= 0, u["cnt"][np.maximum(u["path"], 0)] if N else 0, 1)
    allow = 2.0 * np.abs(u["dv64"]) * (rr.gamma(per_frame - 1) + 2 * rr.U)[:, None]
    err = np.abs(out["dv"][b].astype(np.float64) - u["dv64"])
    assert (err <= allow).all(), (label, b, "dv against float64")
    f_dv = float((err / np.where(allow > 0, allow, 1.0)).max())
    return ulp_m, ulp_dv, f_dx, f_m, f_dv


def _figure(label, figs):
    f = np.array(figs, dtype=np.float64).max(axis=0)
    print("FIGURE %s: quotient %d ulp, dv %d ulp from the float32 restatement; worst error / allowed against float64: dx %.4f, m %.4f, "
          "dv %.4f" % (label, f[0], f[1], f[2], f[3], f[4]))


def shape_case(which, device):
    """One shape of ``SHAPES`` under every duration pattern that fits it and every way of naming T."""
    from tacotron2_amd import alignment
    N, S, C, heavy = SHAPES[which]
    figs, first = [(0, 0, 0.0, 0.0, 0.0)], True
    for pattern in PATTERNS:
        d = durations(N, S, pattern, heavy)
        if d is None:
            continue
        total = int(d.sum())
        many = N <= 65 or first                                              # every T on the small shapes, on one pattern of the large
        first = False
        for i, T in enumerate(t_variants(d) if many else [total]):
            u = utterance(tuple(int(v) for v in d), C, T, WEIGHTS[pattern])
            out = run([u], device, T, offset=(N + S + i) % 4, pad=i % 3, dur_dtype=torch.int64 if i % 2 else torch.int32, lengths=i % 3 != 0)
            figs.append(check(u, out, 0, "%s %s T %d" % (SHAPES[which][:3], pattern, T)))
            if T == total:                                                   # T = None is the longest of the batch
                dt, xt = _t(u["d"]).to(torch.int32).to(device).unsqueeze(0), _t(u["x"]).to(device).unsqueeze(0)
                path, tl = alignment.durations_to_path(dt)
                y, tl2 = alignment.length_regulate(xt, dt)
                assert tuple(y.shape) == (1, total, C) and tuple(path.shape) == (1, total)
                assert np.array_equal(path.cpu().numpy()[0], u["path"]) and int(tl[0]) == int(tl2[0]) == u["Tb"]
                assert np.array_equal(bits(y.cpu().numpy()[0]), bits(u["y"]))
    _figure("shape %s" % (SHAPES[which][:3],), figs)


def overflowing_sums(device):
    """Durations that sum above 2^31 (int32) and above 2^40 (int64) with T = 16 give T_b = 16."""
    from tacotron2_amd import native as nv
    for dtype, big in ((torch.int32, 2 ** 31 - 1), (torch.int64, 2 ** 40)):
        d = torch.tensor([[3, big, big, 5], [big, 0, 1, big], [1, 2, 3, 4]], dtype=dtype).to(device)
        path, tl, ends = (torch.full(s, 0x7f7f7f7f, dtype=torch.int32).to(device) for s in ((3, 16), (3,), (3, 4)))
        totals = torch.zeros(3, dtype=torch.int64).to(device)
        nv.durations_to_path(d, None, 16, path, tl, ends, totals)
        sat = min(big, 2 ** 31 - 1)
        assert tl.tolist() == [16, 16, 10] and totals.tolist() == [8 + 2 * sat, 1 + 2 * sat, 10]
        assert path.tolist() == [[0] * 3 + [1] * 13, [0] * 16, [0, 1, 1, 2, 2, 2, 3, 3, 3, 3] + [-1] * 6]
        assert ends.tolist() == [[3, 16, 16, 16], [16, 16, 16, 16], [1, 3, 6, 10]]


def ragged_utts(T, C=80, wkind="frac"):
    out = []
    for i, N in enumerate(RAGGED_N):
        d = np.zeros(0, np.int64) if N == 0 else durations(N, 2 * N + 3, "zeros" if N >= 5 else "ones", seed=i)
        out.append(utterance(tuple(int(v) for v in d), C, T, wkind, seed=i))
    return out


def ragged_equals_alone(device):
    """A ragged batch of six gives each utterance the bits it gives alone, at another stride and offset; two calls agree; the
    junk beyond N_b (large and negative durations, 1e30) is never read."""
    T = 2 * 130 + 3
    for T_ in (T, 100):                                                      # 100 cuts the two longest
        utts = ragged_utts(T_)
        one, two = run(utts, device, T_, offset=1, pad=2), run(utts, device, T_, offset=1, pad=2)
        for k in one:
            assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), k
        figs = []
        for b, u in enumerate(utts):
            figs.append(check(u, one, b, "ragged T %d" % T_))
            alone = run([u], device, T_, offset=b % 4, pad=b % 3 + (u["N"] == 0))
            n = u["N"]
            for k in ("path", "y", "dv"):
                assert np.array_equal(bits(one[k][b]) if k != "path" else one[k][b], bits(alone[k][0]) if k != "path" else alone[k][0]), (b, k)
            for k in ("dx", "m", "num", "den", "ends"):
                assert np.array_equal(one[k][b, :n].view(np.int32), alone[k][0, :n].view(np.int32)), (b, k)
            assert one["t_lengths"][b] == alone["t_lengths"][0]
        _figure("ragged batch of six, T %d" % T_, figs)


def many_short(device):
    """300 utterances of 1 to 11 tokens: more workgroups than compute units."""
    g = np.random.RandomState(3)
    T, utts = 24, []
    for i in range(300):
        d = g.randint(0, 4, size=1 + i % 11)
        utts.append(utterance(tuple(int(v) for v in d), 5, T, "flags", seed=i))
    out = run(utts, device, T, offset=3, pad=1)
    _figure("300 short utterances", [check(u, out, b, "many short") for b, u in enumerate(utts)])


def pooling_forms(device):
    """No weights, 0/1 flags and fractional weights through the public call; C = 1 as (B, T) and as (B, T, 1) agree bit for bit;
    a token whose frames all weigh 0 gives m = 0 and dv = 0 there."""
    from tacotron2_amd import alignment
    for wkind in (None, "flags", "frac"):
        d = durations(9, 40, "zeros")
        u = utterance(tuple(int(v) for v in d), 1, 40, wkind)
        dt, vt = _t(u["d"]).to(device).unsqueeze(0), _t(u["v"]).to(device).unsqueeze(0)
        wt = None if u["w"] is None else _t(u["w"]).to(device).unsqueeze(0)
        leaves = [vt[:, :, 0].clone().requires_grad_(True), vt.clone().requires_grad_(True)]
        res = [alignment.token_average(leaf, dt, None, wt) for leaf in leaves]
        assert tuple(res[0].shape) == (1, 9) and tuple(res[1].shape) == (1, 9, 1)
        assert np.array_equal(bits(res[0].detach().cpu().numpy()), bits(res[1].detach().cpu().numpy()[:, :, 0]))
        assert rr.ulps(res[0].detach().cpu().numpy()[0], u["p32"]["m"][:, 0]).max() <= MAX_ULPS
        gt = _t(u["g"]).to(device).unsqueeze(0)
        (res[0] * gt[:, :, 0]).sum().backward()
        (res[1] * gt).sum().backward()
        assert np.array_equal(bits(leaves[0].grad.cpu().numpy()), bits(leaves[1].grad.cpu().numpy()[:, :, 0]))
        assert rr.ulps(leaves[0].grad.cpu().numpy()[0], u["dv32"][:, 0]).max() <= MAX_ULPS
        if wkind is not None:
            dead = [n for n in range(9) if (u["path"] == n).any() and u["p32"]["den"][n] == 0]
            assert dead, "the case holds a token whose frames all weigh 0"
            for n in dead:
                assert not bits(res[0].detach().cpu().numpy()[0, n]).any() and not bits(leaves[0].grad.cpu().numpy()[0, u["path"] == n]).any()
        # the values 1: num and den are the same chain of adds, so the mean is exactly 1 wherever den > 0
        ones = alignment.token_average(torch.ones_like(vt), dt, None, wt)
        has = u["p32"]["den"] > 0
        assert (ones.cpu().numpy()[0, :, 0] == np.where(has, 1.0, 0.0)).all()


def round_trip(device):
    """durations_to_path(monotonic_align(s)[0]) is the path monotonic_align returns (section 18), bit for bit."""
    import align_cases
    from tacotron2_amd import alignment
    mats = align_cases.ragged_mats()
    tl, nl = [m.shape[0] for m in mats], [m.shape[1] for m in mats]
    s = torch.full((len(mats), max(tl), max(nl)), -1e30)
    for b, m in enumerate(mats):
        s[b, :tl[b], :nl[b]] = torch.from_numpy(m)
    dur, _, path = alignment.monotonic_align(s.to(device), tl, nl, return_path=True)
    for T in (None, max(tl)):
        got, frames = alignment.durations_to_path(dur, nl, T)
        assert torch.equal(got, path) and frames.tolist() == tl
    got, frames = alignment.durations_to_path(dur.long(), torch.tensor(nl).to(device), max(tl) + 2)     # lengths on the device
    assert torch.equal(got[:, :max(tl)], path) and (got[:, max(tl):] == -1).all() and frames.tolist() == tl


def planted_identity(device):
    """x = one-hot token ids: y's argmax is the path, and token_average(y, d) gives x back exactly on tokens with d >= 1."""
    from tacotron2_amd import alignment
    d = torch.from_numpy(np.stack([durations(12, 40, "zeros"), durations(12, 33, "ones")])).to(device)
    x = torch.eye(12).unsqueeze(0).repeat(2, 1, 1).to(device)
    y, tl = alignment.length_regulate(x, d, [12, 9])
    path, tl2 = alignment.durations_to_path(d, [12, 9])
    assert torch.equal(tl, tl2) and tuple(y.shape) == (2, int(tl.max()), 12)
    for b in range(2):
        n = int(tl[b])
        assert torch.equal(y[b, :n].argmax(dim=1).to(torch.int32), path[b, :n]) and not y[b, n:].any()
    back = alignment.token_average(y, d, [12, 9])
    live = (d > 0) & (torch.arange(12).to(device)[None, :] < torch.tensor([12, 9]).to(device)[:, None])
    assert torch.equal(back[live], x[live]) and not back[~live].any()


def autograd(device):
    """Both functions through torch.autograd against the native entries: a random g, the expanded gradient of .sum().backward(),
    a non-contiguous x, (N, C) as a batch of one, T = int cutting an utterance, and LengthRegulator with float durations."""
    from tacotron2_amd import alignment
    utts = ragged_utts(100, C=7)
    out = run(utts, device, 100)
    B, N = len(utts), max(u["N"] for u in utts)
    nl = [u["N"] for u in utts]
    d, x = torch.zeros(B, N, dtype=torch.int32), torch.zeros(B, N, 7)
    dy, v, w, g = torch.zeros(B, 100, 7), torch.zeros(B, 100, 7), torch.zeros(B, 100), torch.zeros(B, N, 7)
    for b, u in enumerate(utts):
        d[b, :nl[b]], x[b, :nl[b]], g[b, :nl[b]] = _t(u["d"]).int(), _t(u["x"]), _t(u["g"])
        dy[b], v[b], w[b] = _t(u["dy"]), _t(u["v"]), _t(u["w"])
    d, x, dy, v, w, g = (t.to(device) for t in (d, x, dy, v, w, g))
    x = torch.nan_to_num(x, nan=2.0, posinf=3.0, neginf=-3.0)               # a product with dy follows
    leaf = x.clone().requires_grad_(True)
    y, tl = alignment.length_regulate(leaf, d, nl, 100)
    assert y.grad_fn is not None and not tl.requires_grad and tl.tolist() == [u["Tb"] for u in utts]
    with torch.no_grad():
        assert alignment.length_regulate(leaf, d, nl, 100)[0].grad_fn is None
    (y * dy).sum().backward()
    assert np.array_equal(bits(leaf.grad.cpu().numpy()), bits(out["dx"]))
    leaf.grad = None
    alignment.length_regulate(leaf, d, nl, 100)[0].sum().backward()         # a gradient of stride (0, 0, 0) is copied
    counts = torch.from_numpy(np.stack([np.pad(u["cnt"], (0, N - u["N"])) for u in utts])).to(device)
    assert torch.equal(leaf.grad, counts[:, :, None].expand(B, N, 7).float())
    xt = x.transpose(1, 2).contiguous().transpose(1, 2)                     # not contiguous: made so
    assert not xt.is_contiguous() and torch.equal(alignment.length_regulate(xt, d, nl, 100)[0], y.detach())
    one, tl1 = alignment.length_regulate(x[2, :nl[2]], d[2, :nl[2]].long())  # (N, C) and (N,): a batch of one, T = None
    assert tuple(one.shape) == (1, utts[2]["Tb"], 7) and torch.equal(one[0], y.detach()[2, :utts[2]["Tb"]])
    vl = v.clone().requires_grad_(True)
    m = alignment.token_average(vl, d, nl, w)
    assert np.array_equal(bits(m.detach().cpu().numpy()), bits(out["m"]))
    (m * g).sum().backward()
    assert np.array_equal(bits(vl.grad.cpu().numpy()), bits(out["dv"]))
    vl.grad = None
    alignment.token_average(vl, d, nl, w).sum().backward()
    assert torch.isfinite(vl.grad).all()
    # the module: integer durations pass through, float ones are divided by the pace and rounded
    assert not list(alignment.LengthRegulator().parameters())
    assert torch.equal(alignment.LengthRegulator(max_len=100)(x, d, nl)[0], y.detach())
    fd = torch.tensor([[0.4, 1.5, 2.6, -3.0, 0.5]]).to(device)
    x5 = torch.randn(1, 5, 3).to(device).requires_grad_(True)
    for pace, want in ((0.5, [1, 3, 5, 0, 1]), (1.0, [0, 2, 3, 0, 0]), (2.0, [0, 1, 1, 0, 0])):
        y5, t5 = alignment.LengthRegulator(pace=pace)(x5, fd)
        ref = torch.repeat_interleave(x5.detach()[0], torch.tensor(want).to(device), dim=0)
        assert t5.tolist() == [sum(want)] and torch.equal(y5.detach()[0], ref)
        x5.grad = None
        y5.sum().backward()
        assert x5.grad[0, :, 0].tolist() == [float(k) for k in want]
    assert alignment.LengthRegulator(rounding=False)(x5, fd)[1].tolist() == [3]


def refusals(device):
    """Every refusal of section 21.6 by its message."""
    import pytest
    from tacotron2_amd import alignment
    x, d = torch.zeros(2, 4, 3).to(device), torch.ones(2, 4, dtype=torch.int32).to(device)
    f, t = alignment.length_regulate, alignment.token_average
    with pytest.raises(TypeError, match="length_regulate: expected a float32 tensor"):
        f(x.double(), d)
    with pytest.raises(TypeError, match="length_regulate: expected int32 or int64 durations"):
        f(x, d.float())
    with pytest.raises(ValueError, match=r"length_regulate: expected \(B, N, C\) or \(N, C\) tokens"):
        f(x[0, 0], d[0])
    with pytest.raises(ValueError, match=r"length_regulate: expected durations of shape \(2, 4\)"):
        f(x, d[:, :3])
    with pytest.raises(ValueError, match="length_regulate: 513 channels exceed the limit of 512"):
        f(torch.zeros(1, 2, 513).to(device), d[:1, :2])
    with pytest.raises(ValueError, match="length_regulate: 1025 tokens exceed the limit of 1024"):
        f(torch.zeros(1, 1025, 1).to(device), torch.ones(1, 1025, dtype=torch.int32).to(device))
    with pytest.raises(ValueError, match=r"length_regulate: utterance 1: 5 tokens do not lie in \[0, 4\]"):
        f(x, d, [4, 5])
    with pytest.raises(ValueError, match=r"length_regulate: utterance 0: -1 tokens do not lie in \[0, 4\]"):
        f(x, d, [-1, 4])
    with pytest.raises(ValueError, match="length_regulate: n_1 lengths for a batch of 2"):
        f(x, d, [4])
    for T in (-1, 65537, 2.0, True):
        with pytest.raises(ValueError, match=r"length_regulate: T must be None or an int in \[0, 65536\]"):
            f(x, d, None, T)
    neg = d.clone()
    neg[1, 2] = -1
    with pytest.raises(ValueError, match="length_regulate: negative durations"):
        f(x, neg)
    with pytest.raises(ValueError, match="durations_to_path: negative durations"):
        alignment.durations_to_path(neg)
    assert f(x, neg, [4, 2])[1].tolist() == [4, 2]                          # beyond N_b nothing is read
    y, tl = f(x + 1.0, neg, None, 6)                                        # T = int: marked on the device, not refused
    assert tl.tolist() == [4, -1] and not y[1].any() and y[0, :4].all() and not y[0, 4:].any()
    assert alignment.durations_to_path(neg, None, 3)[0].tolist() == [[0, 1, 2], [-1, -1, -1]]
    with pytest.raises(ValueError, match="length_regulate: durations sum to 70000 frames, more than the limit of 65536"):
        f(x, d * 17500)
    y, tl = f(x, d * 0)                                                     # an all-zero batch: T = 0 and an empty y
    assert tuple(y.shape) == (2, 0, 3) and tl.tolist() == [0, 0]
    v = torch.zeros(2, 6, 3).to(device)
    with pytest.raises(TypeError, match="token_average: expected float32 values"):
        t(v.double(), d)
    with pytest.raises(TypeError, match="token_average: expected int32 or int64 durations"):
        t(v, [[1]])
    with pytest.raises(ValueError, match=r"token_average: expected \(B, T\) or \(B, T, C\) values"):
        t(v[0, 0], d)
    with pytest.raises(ValueError, match=r"token_average: expected durations \(2, N\)"):
        t(v, d[:1])
    with pytest.raises(TypeError, match="token_average: expected float32 weights"):
        t(v, d, None, torch.ones(2, 6, dtype=torch.float64).to(device))
    with pytest.raises(ValueError, match=r"token_average: expected weights of shape \(2, 6\)"):
        t(v, d, None, torch.ones(2, 5).to(device))
    with pytest.raises(ValueError, match="token_average: 2 frames and 513 channels exceed the limits"):
        t(torch.zeros(1, 2, 513).to(device), d[:1])
    with pytest.raises(ValueError, match=r"token_average: utterance 0: 9 tokens do not lie in \[0, 4\]"):
        t(v, d, [9, 1])
    assert not t(v + 1.0, neg)[1].any() and t(v + 1.0, neg)[0].all()       # no read-back here: a marked utterance gives zeros
    with pytest.raises(ValueError, match="LengthRegulator: the pace must be a positive number"):
        alignment.LengthRegulator(pace=0.0)
    with pytest.raises(ValueError, match="LengthRegulator: max_len must be None or an int"):
        alignment.LengthRegulator(max_len=-2)
