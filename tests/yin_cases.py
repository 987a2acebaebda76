"""The cases and assertions the CPU file (csrc/yin.hip on the host stand-in) and the GPU file (the MI355X) of the YIN tests share:
every check takes a ``device`` and runs tacotron2_amd.native / tacotron2_amd.audio on tensors of that device."""
import numpy as np
import torch

import yin_ref as yr
from tacotron2_amd import audio, native

POISON = -777.0
PERIODS = (27, 28, 40, 63, 100, 101, 200, 255, 256, 300, 367, 368)
DEFAULT = dict(sr=22050, frame_length=1024, hop_length=256, fmin=60.0, fmax=800.0, threshold=0.1)
SMALL = dict(sr=60, frame_length=64, hop_length=16, fmin=2.0, fmax=30.0, threshold=0.1)          # lags 2 .. 30: below one wave
ODD = dict(sr=8000, frame_length=256, hop_length=64, fmin=80.0, fmax=500.0, threshold=0.15)      # 101 lags: no multiple of 64
TAIL = dict(sr=60, frame_length=70, hop_length=7, fmin=2.0, fmax=30.0, threshold=0.1)            # W = 35: no multiple of 4
LONG = dict(sr=48000, frame_length=2048, hop_length=512, fmin=50.0, fmax=1000.0, threshold=0.1)  # 961 lags: a lane owns four


def run(signals, device, geo, offset=0, pad=3):
    """The native launch on poisoned outputs for a ragged batch of float32 numpy signals, without and with the d' slab.  The
    batch is a view into a wider buffer that starts ``offset`` floats into its rows and holds 1e30 wherever no utterance is.
    -> (f0, voiced, aperiodicity, slab) as numpy, after checking that the two calls agree bit for bit, that every element was
    written and that frames at and beyond an utterance's count are 0 / False / 0."""
    B, lens = len(signals), [len(s) for s in signals]
    T = max(lens)
    buf = torch.full((B, offset + T + pad), 1e30)
    for b, s in enumerate(signals):
        buf[b, offset:offset + lens[b]] = torch.from_numpy(s)
    x = buf.to(device)[:, offset:offset + T]
    n = torch.tensor(lens, dtype=torch.int32).to(device)
    L, hop = geo["frame_length"], geo["hop_length"]
    tau_min, tau_max = native.yin_plan(geo["sr"], L, hop, geo["fmin"], geo["fmax"])
    assert (L // 2, tau_min, tau_max) == yr.geometry(geo["sr"], L, geo["fmin"], geo["fmax"])
    frames = T // hop + 1

    def outputs():
        return (torch.full((B, frames), POISON, device=device), torch.full((B, frames), 0xEE, dtype=torch.uint8, device=device),
                torch.full((B, frames), POISON, device=device))
    f0, vo, ap = outputs()
    native.yin(x, n, L, hop, tau_min, tau_max, geo["sr"], geo["threshold"], f0, vo, ap)
    f0s, vos, aps = outputs()
    slab = torch.full((B, frames, tau_max + 2), POISON, device=device)
    native.yin(x, n, L, hop, tau_min, tau_max, geo["sr"], geo["threshold"], f0s, vos, aps, slab)
    f0, vo, ap, f0s, vos, aps, slab = (t.cpu().numpy() for t in (f0, vo, ap, f0s, vos, aps, slab))
    assert np.array_equal(f0.view(np.int32), f0s.view(np.int32)) and np.array_equal(ap.view(np.int32), aps.view(np.int32))
    assert np.array_equal(vo, vos) and vo.max() <= 1
    assert not (f0 == POISON).any() and not (ap == POISON).any() and not (slab == POISON).any()
    for b in range(B):
        c = yr.frame_count(lens[b], hop)
        assert not f0[b, c:].any() and not vo[b, c:].any() and not ap[b, c:].any() and not slab[b, c:].any()
    return f0, vo.astype(bool), ap, slab


def check_utterance(x, geo, f0, voiced, ap, slab, name=""):
    """Items 2 and 3 of one utterance, and the frames of item 4: d' of every lag of every frame within the bound of the float64
    restatement; the rule applied to the kernel's own slab gives the kernel's lag and flag exactly, its aperiodicity bit for bit,
    its shift and f0 within the bound the slab's three values give; where the restatement's decision has margin the kernel's lag
    and flag are the restatement's.  -> (worst d' error over bound, frames, decided frames)."""
    sr, thr = geo["sr"], geo["threshold"]
    ref = yr.analyse(x, **geo)
    W, tau_min, tau_max = ref["W"], ref["tau_min"], ref["tau_max"]
    count = ref["dprime"].shape[0]
    tol = yr.bound(W, tau_max)
    want, got = ref["dprime"], slab[:count].astype(np.float64)
    assert np.array_equal(got[want == 0.0], want[want == 0.0])
    rel = np.abs(got - want) / np.where(want > 0, want, 1.0)
    worst = float(rel.max() / tol)
    assert worst <= 1.0, (name, worst)
    n_decided = 0
    for t in range(count):
        row = slab[t]
        tau, flag = yr.choose(row, tau_min, tau_max, thr)
        assert bool(voiced[t]) == flag, (name, t)
        assert np.float32(ap[t]).view(np.int32) == np.float32(row[tau]).view(np.int32), (name, t, tau)
        shift = yr.refine(row[tau - 1], row[tau], row[tau + 1])
        ds = yr.shift_bound(row[tau - 1], row[tau], row[tau + 1])
        p = tau + shift
        dper = ds + 2 * yr.U * p                                        # the period: the shift's bound and one rounding of the sum
        df0 = sr / (p - dper) - sr / p + 2 * yr.U * sr / (p - dper)     # the quotient: one rounding, and its operand's
        assert abs(float(f0[t]) - sr / p) <= df0, (name, t, tau, shift, float(f0[t]), sr / p, df0)
        if yr.decided(want[t], tau_min, tau_max, thr, tol):
            n_decided += 1
            assert (tau, flag) == (int(ref["tau"][t]), bool(ref["voiced"][t])), (name, t)
    return worst, count, n_decided


def check_batch(signals, device, geo, name, offset=0, min_decided=None):
    f0, vo, ap, slab = run(signals, device, geo, offset)
    frames = decided = 0
    worst = 0.0
    for b, x in enumerate(signals):
        w, c, dcd = check_utterance(x, geo, f0[b], vo[b], ap[b], slab[b], "%s[%d]" % (name, b))
        left = 1.0 - dcd / c
        print("FIGURE %s[%d]: %d samples, %d frames, worst d' error / bound %.4f, left out as undecided %.1f %%"
              % (name, b, len(x), c, w, 100 * left))
        if min_decided is not None:
            assert left <= 1.0 - min_decided, (name, b, left)
        worst, frames, decided = max(worst, w), frames + c, decided + dcd
    print("FIGURE %s: %d frames, worst d' error / bound %.4f, undecided %.1f %% overall" % (name, frames, worst,
                                                                                           100 * (1 - decided / frames)))
    assert 1 - decided / frames <= 0.10, (name, decided, frames)              # a case leaves out a tenth of its frames at most
    return f0, vo, ap, slab


def periodic_structure(device):
    """Item 1: exact integer periods at the default geometry, one ragged batch.  On every interior frame the frame is voiced, the lag
    is exactly P, the aperiodicity is exactly 0 and |tau + shift - P| <= 1/2; tau + shift is read back from f0 = sr / (tau + shift),
    two float32 roundings away."""
    geo = DEFAULT
    L, hop, sr = geo["frame_length"], geo["hop_length"], geo["sr"]
    signals = [yr.periodic(P, 2560 + 7 * i) for i, P in enumerate(PERIODS)]
    f0, vo, ap, slab = run(signals, device, geo)
    _, tau_min, tau_max = yr.geometry(sr, L, geo["fmin"], geo["fmax"])
    for b, P in enumerate(PERIODS):
        n = len(signals[b])
        ref = yr.analyse(signals[b], **geo)
        interior = [t for t in range(yr.frame_count(n, hop)) if t * hop - L // 2 >= 0 and t * hop + L // 2 <= n]
        assert len(interior) >= 6
        for t in interior:
            assert ref["voiced"][t] and ref["tau"][t] == P and ref["aperiodicity"][t] == 0.0
            assert abs(ref["tau"][t] + ref["shift"][t] - P) <= 0.5
            assert vo[b, t] and ap[b, t] == 0.0
            assert yr.choose(slab[b, t], tau_min, tau_max, geo["threshold"]) == (P, True)
            assert abs(sr / float(f0[b, t]) - P) <= 0.5 + 3 * yr.U * (P + 0.5)
        check_utterance(signals[b], geo, f0[b], vo[b], ap[b], slab[b], "period %d" % P)


def glide_signals():
    return [yr.glide(seed) for seed in range(6)]


def small_signals():
    """The small geometry (L = 64, hop 16): n < hop (one frame), n < L / 2, n an exact multiple of hop and one more, noise, short
    periods, one sample.  (All zeros, where every comparison is an exact tie, is ``all_zero``'s and the ragged batch's.)"""
    g = np.random.RandomState(7)
    return [g.randn(5).astype(np.float32), g.randn(20).astype(np.float32), g.randn(160).astype(np.float32),
            g.randn(161).astype(np.float32), yr.periodic(7, 150, 1), yr.periodic(12, 97, 2),
            (yr.periodic(9, 130, 3) + 0.05 * g.randn(130)).astype(np.float32), g.randn(1).astype(np.float32)]


def all_zero(device, geo=SMALL):
    """Every d' = 1: unvoiced, tau = tau_min, shift 0."""
    f0, vo, ap, slab = run([np.zeros(100, np.float32)], device, geo)
    _, tau_min, _ = yr.geometry(geo["sr"], geo["frame_length"], geo["fmin"], geo["fmax"])
    c = yr.frame_count(100, geo["hop_length"])
    assert (slab[0, :c] == 1.0).all() and not vo[0].any() and (ap[0, :c] == 1.0).all()
    assert (f0[0, :c] == np.float32(geo["sr"]) / np.float32(tau_min)).all()


def ragged_equals_alone(signals, device, geo, offset=1):
    """A ragged batch gives each utterance the bits it gives alone (at another alignment of its row too), and two calls agree."""
    signals = list(signals) + [np.zeros(len(signals[0]) + 3, np.float32)]
    one = run(signals, device, geo, offset)
    two = run(signals, device, geo, offset)
    for a, b in zip(one, two):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for b, x in enumerate(signals):
        alone = run([x], device, geo, (offset + b) % 4)
        c = alone[0].shape[1]
        for whole, own in zip(one, alone):
            assert np.array_equal(whole[b, :c].view(np.uint8), own[0].view(np.uint8)), b


def module_equals_native(signals, device, geo):
    """audio.yin on the padded batch: the bits of the native calls, with and without the slab; a (T,) signal is a batch of one."""
    f0, vo, ap, slab = run(signals, device, geo)
    lens = [len(s) for s in signals]
    x = torch.zeros(len(signals), max(lens))
    for b, s in enumerate(signals):
        x[b, :lens[b]] = torch.from_numpy(s)
    x = x.to(device).requires_grad_(True)
    a = audio.yin(x, lens, **geo)
    b = audio.yin(x, lens, return_dprime=True, **geo)
    assert len(a) == 3 and len(b) == 4 and a[1].dtype == torch.bool and all(t.grad_fn is None and not t.requires_grad for t in b)
    for got, want in zip(b, (f0, vo, ap, slab)):
        assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8))
    for got, again in zip(a, b):
        assert torch.equal(got, again)
    single = audio.yin(x.detach()[0, :lens[0]], **geo)
    c = single[0].shape[1]
    assert single[0].shape == (1, yr.frame_count(lens[0], geo["hop_length"])) and torch.equal(single[0][0], a[0][0, :c])


def metric_tracks(seed=0, B=4, Ta=30, Tb=37):
    """Random F0 tracks with flags, lengths and monotone paths; the last pair has no both-voiced step."""
    g = np.random.RandomState(seed)
    fa, fb = g.uniform(80, 400, size=(B, Ta)), g.uniform(80, 400, size=(B, Tb))
    va, vb = g.rand(B, Ta) < 0.7, g.rand(B, Tb) < 0.7
    vb[-1] = False
    la, lb = [Ta, Ta - 4, 9, Ta], [Tb - 2, Tb, 5, Tb]
    paths = []
    for b in range(B):
        i = j = 0
        p = [(0, 0)]
        while (i, j) != (la[b] - 1, lb[b] - 1):
            moves = [(di, dj) for di, dj in ((1, 1), (1, 0), (0, 1)) if i + di < la[b] and j + dj < lb[b]]
            di, dj = moves[g.randint(len(moves))]
            i, j = i + di, j + dj
            p.append((i, j))
        paths.append(p)
    return fa, va, fb, vb, la, lb, paths


def check_metrics(device):
    """audio.f0_metrics against the restatement's float64 metrics, with and without a path, the NaN rule, identical inputs."""
    fa, va, fb, vb, la, lb, paths = metric_tracks()
    B, Lp = len(la), max(len(p) for p in paths)
    path = np.full((B, Lp, 2), -1, dtype=np.int32)
    for b, p in enumerate(paths):
        path[b, :len(p)] = np.array(p)
    steps = torch.tensor([len(p) for p in paths], dtype=torch.int32).to(device)
    t = [torch.from_numpy(v).to(device) for v in (fa.astype(np.float32), va, fb.astype(np.float32), vb)]
    fa32, fb32 = fa.astype(np.float32), fb.astype(np.float32)
    for with_path in (True, False):
        if with_path:
            got = audio.f0_metrics(*t, len_a=la, len_b=lb, path=torch.from_numpy(path).to(device), steps=steps)
        else:
            got = audio.f0_metrics(*t, len_a=la, len_b=lb)
        for b in range(B):
            pairs = paths[b] if with_path else [(i, i) for i in range(min(la[b], lb[b]))]
            want = yr.metrics(fa32[b], va[b], fb32[b], vb[b], pairs)
            assert int(got["voiced_steps"][b]) == want["voiced_steps"]
            for key in ("f0_rmse_cents", "f0_corr", "vuv_error", "gross_pitch_error"):
                g_, w_ = float(got[key][b]), want[key]
                assert (np.isnan(g_) and np.isnan(w_)) or abs(g_ - w_) <= 1e-9 * max(1.0, abs(w_)), (with_path, b, key, g_, w_)
        assert np.isnan(float(got["f0_rmse_cents"][-1])) and np.isnan(float(got["f0_corr"][-1]))
        assert np.isnan(float(got["gross_pitch_error"][-1])) and int(got["voiced_steps"][-1]) == 0
        assert not np.isnan(float(got["vuv_error"][-1]))
    same = audio.f0_metrics(t[0], t[1], t[0].clone(), t[1].clone())
    for b in range(B):
        assert float(same["f0_rmse_cents"][b]) == 0.0 and abs(float(same["f0_corr"][b]) - 1.0) <= 1e-12
        assert float(same["vuv_error"][b]) == 0.0 and float(same["gross_pitch_error"][b]) == 0.0


def write_wav(path, x, sr):
    """x scaled to half of full scale, as 16-bit PCM."""
    from scipy.io.wavfile import write
    write(path, sr, np.round(np.asarray(x, dtype=np.float64) / np.abs(x).max() * 16000.0).astype(np.int16))


def pulse_train(P, n):
    """A smooth pulse of exact integer period P: strongly periodic, so that every frame that lies inside the signal is voiced."""
    k = np.arange(n) % P
    return np.exp(-0.5 * ((k - P / 2.0) / (P / 10.0)) ** 2) - 0.2


def refusals(device):
    """The refusals of section 17.1, each by its message."""
    import pytest
    x = torch.zeros(2, 4000).to(device)
    cases = [(dict(frame_length=600), "W \\+ tau_max \\+ 1 exceeds frame_length"),          # 300 + 368 + 1 > 600
             (dict(fmax=20000.0), "tau_min = floor\\(sr / fmax\\) must be at least 2"),
             (dict(fmin=800.0, fmax=800.0), "fmin must be below fmax"),
             (dict(fmin=900.0, fmax=800.0), "fmin must be below fmax"),
             (dict(frame_length=1025), "frame_length must be even"),
             (dict(hop_length=0), "hop_length must be at least 1"),
             (dict(frame_length=8192, fmin=10.0), "frame_length must not exceed 4096")]
    for kw, msg in cases:
        with pytest.raises((ValueError, native.NativeError), match=msg):
            audio.yin(x, **kw)
    with pytest.raises(TypeError, match="float32"):
        audio.yin(x.double())
    with pytest.raises(TypeError, match="float32"):
        audio.yin([0.0, 1.0])
    with pytest.raises(ValueError, match="unit stride along time"):
        audio.yin(x[:, ::2])
    with pytest.raises(ValueError, match="unit stride along time"):
        audio.yin(torch.zeros(4000, 2).to(device).t())
    with pytest.raises(ValueError, match=r"\(B, T\) or \(T,\)"):
        audio.yin(torch.zeros(1, 2, 4000).to(device))
    for bad in ([0, 4000], [4000, 4001]):
        with pytest.raises(ValueError, match=r"lengths must lie in \[1, 4000\]"):
            audio.yin(x, bad)
    with pytest.raises(ValueError, match="lengths for a batch"):
        audio.yin(x, [4000])
