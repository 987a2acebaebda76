"""audio.yin on the MI355X beside two statements of the same estimator: float32 torch ops on the GPU (unfold, the difference
function from two running energies and an rfft cross-correlation, cumsum, masks) and the float64 numpy restatement of the tests on
the CPU.  One JSON line.

    python tools/bench_yin.py [--reps 5] [--inner 20] [--cases b1,b16] [--no-baselines] [--out F]

Writes the line to profiles/yin_bench.json as well (``--out`` names another file).

Cases: B = 1 at 870 frames (222 464 samples), and B = 16 ragged: synth_lengths(16, 1234) frames, (frames - 1) hop samples each.  The
signals are five harmonics of a slowly gliding pitch plus noise, at the default geometry (22 050 Hz, frames of 1024 every 256, 60 to
800 Hz: lags 27 to 368).  For each: ms per call of audio.yin without and with the d' slab (a host clock around `inner` calls that end
in one device synchronise, divided by `inner`; median of `reps` after a warm-up); ms per launch of the kernel (each launch between
a pair of events, mean of `inner`); the torch statement on the same signals, checked against the native call (share of frames
whose voiced flags agree, and the median of |f0 - f0| over frames both call voiced); the numpy restatement of the first utterance,
scaled to the batch's frames.  ratio_* is the baseline's time over the native call without the slab (above 1: the native path is
faster)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_mel_loss import _ms, kernel_times  # noqa: E402
from tacotron2_amd import audio, native  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402

SR, L, HOP, FMIN, FMAX, THR = 22050, 1024, 256, 60.0, 800.0, 0.1


def torch_yin(y, lens, tau_min, tau_max):
    """(f0, voiced) as float32 torch ops, the whole batch per op."""
    B, T = y.shape
    W, nl = L // 2, tau_max + 1
    dev = y.device
    y = torch.where(torch.arange(T, device=dev)[None, :] < lens[:, None], y, torch.zeros((), device=dev))
    fr = torch.nn.functional.pad(y, (W, W + HOP)).unfold(1, L, HOP)[:, :T // HOP + 1]           # (B, frames, L)
    spec = torch.fft.rfft(fr, 2 * L) * torch.fft.rfft(fr[..., :W], 2 * L).conj()
    corr = torch.fft.irfft(spec, 2 * L)[..., :nl + 1]                                             # sum_j f[j] f[j + tau]
    e = torch.nn.functional.pad((fr * fr).cumsum(-1), (1, 0))
    tau = torch.arange(nl + 1, device=dev)
    d = (e[..., W:W + 1] + (e[..., W + tau] - e[..., tau]) - 2.0 * corr).clamp_(min=0.0)
    d[..., 0] = 0.0
    S = d.cumsum(-1)
    dp = torch.where(S > 0, d * tau / S.clamp(min=1e-30), torch.ones((), device=dev))
    dp[..., 0] = 1.0
    mid = dp[..., tau_min:tau_max + 1]
    dip = (mid < THR) & (mid < dp[..., tau_min - 1:tau_max]) & (mid <= dp[..., tau_min + 1:tau_max + 2])
    voiced = dip.any(-1)
    k = torch.where(voiced, dip.float().argmax(-1), mid.argmin(-1)) + tau_min
    dm, d0, dn = (dp.gather(-1, (k + o).unsqueeze(-1)).squeeze(-1) for o in (-1, 0, 1))
    a, b = dm + dn - 2.0 * d0, (dn - dm) * 0.5
    ok = (d0 <= dm) & (d0 <= dn) & (a > 0)
    shift = torch.where(ok, -b / torch.where(ok, a, torch.ones_like(a)), torch.zeros_like(a)).clamp_(-0.5, 0.5)
    return SR / (k.float() + shift), voiced


def signal(n, seed):
    g = np.random.RandomState(seed)
    f = g.uniform(90, 300) * (1.0 + 0.1 * np.sin(2 * np.pi * np.arange(n) / SR * 0.7))
    phase = 2 * np.pi * np.cumsum(f) / SR
    x = sum(np.sin(k * phase + g.uniform(0, 6.28)) / k for k in range(1, 6))
    gate = (np.sin(2 * np.pi * np.arange(n) / SR * 1.3 + g.uniform(0, 6.28)) > -0.3)
    return (0.3 * gate * x + 0.01 * g.randn(n)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--cases", default="b1,b16")
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yin_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tau_min, tau_max = native.yin_plan(SR, L, HOP, FMIN, FMAX)
    res = {"inner": args.inner, "reps": args.reps, "sr": SR, "frame_length": L, "hop_length": HOP, "tau_min": tau_min,
           "tau_max": tau_max, "cases": {}}
    for case in args.cases.split(","):
        frames = [870] if case == "b1" else [int(v) for v in synth_lengths(int(case[1:]), 1234)[1]]
        lens = [(f - 1) * HOP for f in frames]
        B, T = len(lens), max(lens)
        x = torch.zeros(B, T)
        for b, n in enumerate(lens):
            x[b, :n] = torch.from_numpy(signal(n, 10 + b))
        x = x.to(dev)
        dlens = torch.tensor(lens, device=dev)

        def many(fn):
            def run():
                for _ in range(args.inner):
                    fn()
            return run

        t = {"yin": _ms(many(lambda: audio.yin(x, lens, SR, L, HOP, FMIN, FMAX, THR)), args.reps) / args.inner,
             "yin_with_slab": _ms(many(lambda: audio.yin(x, lens, SR, L, HOP, FMIN, FMAX, THR, True)), args.reps) / args.inner}
        kt = kernel_times(many(lambda: audio.yin(x, lens, SR, L, HOP, FMIN, FMAX, THR)), ("yin",))
        kts = kernel_times(many(lambda: audio.yin(x, lens, SR, L, HOP, FMIN, FMAX, THR, True)), ("yin",))
        terms = sum(frames) * (tau_max + 1) * (L // 2)
        r = {"B": B, "frames": [min(frames), max(frames)], "frames_total": sum(frames), "difference_terms": terms,
             "call_ms": {k: round(v, 4) for k, v in t.items()},
             "kernel_ms": {"yin": round(kt["yin"]["ms"] / kt["yin"]["launches"], 4),
                           "yin_with_slab": round(kts["yin"]["ms"] / kts["yin"]["launches"], 4)}}
        r["terms_per_ns"] = round(terms / (r["kernel_ms"]["yin"] * 1e6), 1)
        if not args.no_baselines:
            f0, voiced, _ = audio.yin(x, lens, SR, L, HOP, FMIN, FMAX, THR)
            tf0, tvoiced = torch_yin(x, dlens, tau_min, tau_max)
            valid = torch.arange(f0.shape[1], device=dev)[None, :] < torch.tensor(frames, device=dev)[:, None]
            both = voiced & tvoiced & valid
            r["torch_fp32_ms"] = round(_ms(lambda: torch_yin(x, dlens, tau_min, tau_max), args.reps), 3)
            r["torch_voiced_agreement"] = float(((voiced == tvoiced) & valid).sum() / valid.sum())
            r["torch_median_abs_f0_diff_hz"] = float((f0 - tf0).abs()[both].median()) if bool(both.any()) else None
            import yin_ref
            t0 = time.perf_counter()
            ref = yin_ref.analyse(x[0, :lens[0]].cpu().numpy(), SR, L, HOP, FMIN, FMAX, THR)
            r["numpy_fp64_ms"] = round((time.perf_counter() - t0) * 1e3 * sum(frames) / frames[0], 3)
            r["numpy_voiced_agreement_first_utterance"] = float((ref["voiced"] == voiced[0, :frames[0]].cpu().numpy()).mean())
            r["ratio_to_torch"] = round(r["torch_fp32_ms"] / t["yin"], 1)
            r["ratio_to_numpy"] = round(r["numpy_fp64_ms"] / t["yin"], 1)
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
