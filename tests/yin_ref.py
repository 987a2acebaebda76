"""YIN in float64 numpy, written from DESIGN.md section 17.1 (the definitions of the F0 issue), not from csrc/yin.hip: frames, the
difference function, its cumulative-mean normalisation d', the choice of lag, the parabolic refinement, and the F0 metrics.  The
rule of choice and the refinement take a row of d' of any float type, so the tests also apply them to the kernel's float32 slab."""
import numpy as np

U = 2.0 ** -24                                   # float32 unit roundoff


def geometry(sr, frame_length=1024, fmin=60.0, fmax=800.0):
    """-> (W, tau_min, tau_max)."""
    return frame_length // 2, int(np.floor(sr / fmax)), int(np.ceil(sr / fmin))


def frame_count(n, hop):
    return n // hop + 1


def frames(x, L, hop):
    """(count, L) float64: frame t is x[t hop - L/2 : t hop + L/2] with zeros outside the signal."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    pad = np.concatenate([np.zeros(L // 2), x, np.zeros(L)])
    return np.stack([pad[t * hop:t * hop + L] for t in range(frame_count(n, hop))])


def dprime(fr, tau_max):
    """(count, tau_max + 2) float64: d'(0 .. tau_max + 1) of every frame."""
    W = fr.shape[1] // 2
    d = np.zeros((fr.shape[0], tau_max + 2))
    for tau in range(1, tau_max + 2):
        df = fr[:, :W] - fr[:, tau:tau + W]
        d[:, tau] = (df * df).sum(axis=1)
    S = np.cumsum(d, axis=1)
    tau = np.arange(tau_max + 2, dtype=np.float64)[None, :]
    out = np.where(S > 0, d * tau / np.where(S > 0, S, 1.0), 1.0)
    out[:, 0] = 1.0
    return out


def threshold32(threshold):
    """The threshold as the kernel compares against it: rounded to float32 once."""
    return float(np.float32(threshold))


def choose(dp, tau_min, tau_max, threshold):
    """The rule on one row of d' (comparisons only): -> (tau, voiced)."""
    thr = threshold32(threshold)
    v = dp[tau_min:tau_max + 1]
    dip = (v < thr) & (v < dp[tau_min - 1:tau_max]) & (v <= dp[tau_min + 1:tau_max + 2])
    if dip.any():
        return tau_min + int(np.argmax(dip)), True
    return tau_min + int(np.argmin(v)), False               # argmin takes the first of equals


def refine(dm, d0, dp):
    """shift = -b / a where a > 0 and |b| <= a / 2, else 0, in float64.  |b| <= a / 2 is d0 <= min(dm, dp): tested in that form."""
    dm, d0, dp = float(dm), float(d0), float(dp)
    if not (d0 <= dm and d0 <= dp):
        return 0.0
    a = dm + dp - 2.0 * d0
    b = (dp - dm) / 2.0
    return min(0.5, max(-0.5, -b / a)) if a > 0 else 0.0     # |b| <= a / 2: the clip only takes a rounding back


def decided(dp, tau_min, tau_max, threshold, eps):
    """Whether every comparison the rule makes on the way to its answer on this row holds with both sides moved by the relative
    ``eps`` against it."""
    thr = threshold32(threshold)
    lo, hi = dp * (1.0 - eps), dp * (1.0 + eps)
    r = slice(tau_min, tau_max + 1)
    sure_dip = (hi[r] < thr) & (hi[r] < lo[tau_min - 1:tau_max]) & (hi[r] <= lo[tau_min + 1:tau_max + 2])
    sure_not = (lo[r] > thr) | (lo[r] >= hi[tau_min - 1:tau_max]) | (lo[r] > hi[tau_min + 1:tau_max + 2])
    tau, voiced = choose(dp, tau_min, tau_max, threshold)
    k = tau - tau_min
    if voiced:
        return bool(sure_dip[k] and sure_not[:k].all())
    others = np.delete(lo[r], k)
    return bool(sure_not.all() and (others.size == 0 or hi[tau] < others.min()))


def bound(W, tau_max):
    """The relative error allowed to a float32 d' (DESIGN.md section 17.3): W + 2 roundings in d, as many in the terms of S plus at
    most tau_max additions, a multiply and a divide, and 2 for the second-order terms."""
    return (2 * W + tau_max + 8) * U


def shift_bound(dm, d0, dp):
    """|float32 shift - float64 shift| from the same three float32 values: 6 u max(d') / a, at most 1 (section 17.3)."""
    dm, d0, dp = float(dm), float(d0), float(dp)
    a = dm + dp - 2.0 * d0
    if not (d0 <= dm and d0 <= dp) or not a > 0:             # no refinement on either side: the condition is comparisons alone
        return 0.0
    return min(1.0, 6.0 * U * max(dm, dp) / a)


def analyse(x, sr=22050, frame_length=1024, hop_length=256, fmin=60.0, fmax=800.0, threshold=0.1):
    """-> dict of per-frame arrays: f0, voiced, aperiodicity, tau, shift, and dprime (count, tau_max + 2)."""
    W, tau_min, tau_max = geometry(sr, frame_length, fmin, fmax)
    dp = dprime(frames(x, frame_length, hop_length), tau_max)
    n = dp.shape[0]
    tau, voiced, shift = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.zeros(n)
    for t in range(n):
        tau[t], voiced[t] = choose(dp[t], tau_min, tau_max, threshold)
        shift[t] = refine(dp[t, tau[t] - 1], dp[t, tau[t]], dp[t, tau[t] + 1])
    return {"f0": sr / (tau + shift), "voiced": voiced, "aperiodicity": dp[np.arange(n), tau], "tau": tau, "shift": shift,
            "dprime": dp, "tau_min": tau_min, "tau_max": tau_max, "W": W}


def metrics(f0_a, voiced_a, f0_b, voiced_b, path=None):
    """The F0 figures of one pair in float64; ``path``: a list of (i, j), None: index by index up to the shorter track."""
    if path is None:
        path = [(i, i) for i in range(min(len(f0_a), len(f0_b)))]
    ia, ib = np.array([p[0] for p in path], dtype=np.int64), np.array([p[1] for p in path], dtype=np.int64)
    fa, fb = np.asarray(f0_a, dtype=np.float64)[ia], np.asarray(f0_b, dtype=np.float64)[ib]
    va, vb = np.asarray(voiced_a, dtype=bool)[ia], np.asarray(voiced_b, dtype=bool)[ib]
    both = va & vb
    out = {"vuv_error": float((va != vb).mean()), "voiced_steps": int(both.sum())}
    if not both.any():
        out.update(f0_rmse_cents=float('nan'), f0_corr=float('nan'), gross_pitch_error=float('nan'))
        return out
    fa, fb = fa[both], fb[both]
    cents = 1200.0 * np.log2(fa / fb)
    ca, cb = fa - fa.mean(), fb - fb.mean()
    den = np.sqrt((ca * ca).sum() * (cb * cb).sum())
    out.update(f0_rmse_cents=float(np.sqrt((cents * cents).mean())), f0_corr=float((ca * cb).sum() / den) if den > 0 else float('nan'),
               gross_pitch_error=float((np.abs(fa / fb - 1.0) > 0.2).mean()))
    return out


def periodic(P, n, seed=0):
    """A random waveform of exact integer period P, tiled to n samples, float32."""
    return np.tile(np.random.RandomState(seed).randn(P), n // P + 1)[:n].astype(np.float32)


def glide(seed, n=10240, sr=22050):
    """Five gliding harmonics plus noise, gated into voiced and unvoiced stretches, float32."""
    g = np.random.RandomState(100 + seed)
    f_a = g.uniform(90, 300)
    f_b = f_a * g.uniform(0.85, 1.15)
    t = np.arange(n)
    phase = 2 * np.pi * np.cumsum(f_a + (f_b - f_a) * t / n) / sr
    voiced = sum(np.sin(k * phase + g.uniform(0, 2 * np.pi)) / k for k in range(1, 6))
    gate = np.zeros(n)
    edges = np.sort(g.choice(np.arange(1, 40), size=3, replace=False)) * 256
    gate[edges[0]:edges[1]] = 1.0
    gate[edges[2]:] = 1.0
    return (0.3 * gate * voiced + (0.002 + 0.05 * (1 - gate)) * g.randn(n)).astype(np.float32)
