"""audio.MelCepstralDistortion on the MI355X beside two statements of the same recurrence, one anti-diagonal at a time: float32
torch ops on the GPU and a float32 numpy loop on the CPU.  One JSON line.

    python tools/bench_mcd.py [--reps 5] [--inner 10] [--cases b1,b64] [--no-baselines] [--out F]

Writes the line to profiles/mcd_bench.json as well (``--out`` names another file).

Cases: B = 1 at 870 x 870 frames, and B = 64 ragged: synth_lengths(64, 1234) frames on the first side, each scaled by a factor
drawn from [0.9, 1.1] (clipped to 870) on the second.  The mels are -5 + 2 randn, 80 channels, 13 coefficients.  For each: ms per
call of the module, cost only and with the path, and of the cepstrum kernel alone (a host clock around `inner` calls that end in
one device synchronise, divided by `inner`; median of `reps` after a warm-up); ms per launch of the three kernels (each launch
between a pair of events, mean of `inner`); barrier steps of the DTW launch's longest pair and ns per step; the torch statement on
the same cepstra (cost matrix from differences, skewed once, then pad / pad / minimum / minimum / add per anti-diagonal, the
whole batch per op; no step count, no path); the numpy statement (the same per pair).  Both baselines are checked against the
native cost (max relative difference).  ratio_* is the baseline's time over the native cost-only DTW's call (above 1: the native
path is faster)."""
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

from bench_mel_loss import _ms, kernel_times  # noqa: E402
from tacotron2_amd import audio, native  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402


def torch_dtw(x, y, la, lb):
    """cost (B,) of the recurrence as float32 torch ops, one set per anti-diagonal, the whole batch per op."""
    B, Ta, _ = x.shape
    Tb = y.shape[1]
    dev = x.device
    d = torch.cat([(x[s:s + 4, :, None, :] - y[s:s + 4, None, :, :]).square().sum(-1).sqrt() for s in range(0, B, 4)])
    i = torch.arange(Ta, device=dev)[None, :]
    j = torch.arange(Ta + Tb - 1, device=dev)[:, None] - i
    inf = float("inf")
    dsk = torch.where(((j >= 0) & (j < Tb))[None], d[:, i.expand_as(j), j.clamp(0, Tb - 1)], torch.tensor(inf, device=dev))
    D = torch.empty(Ta + Tb - 1, B, Ta, device=dev)
    D[0] = dsk[:, 0]
    pad = torch.nn.functional.pad
    for t in range(1, Ta + Tb - 1):
        prev1 = D[t - 1]
        up = pad(prev1[:, :-1], (1, 0), value=inf)
        m = torch.minimum(up, prev1)
        if t > 1:
            m = torch.minimum(m, pad(D[t - 2][:, :-1], (1, 0), value=inf))
        torch.add(dsk[:, t], m, out=D[t])
    la, lb = torch.as_tensor(la, device=dev), torch.as_tensor(lb, device=dev)
    return D[la + lb - 2, torch.arange(B, device=dev), la - 1]


def numpy_dtw(a, b):
    """cost of one pair as a float32 numpy anti-diagonal loop."""
    n_a, n_b = a.shape[0], b.shape[0]
    df = a[:, None, :] - b[None, :, :]
    d = np.sqrt((df * df).sum(-1, dtype=np.float32))
    inf = np.float32(np.inf)
    prev2 = np.full(n_a, inf, np.float32)
    prev1 = np.full(n_a, inf, np.float32)
    prev1[0] = d[0, 0]
    for t in range(1, n_a + n_b - 1):
        lo, hi = max(0, t - n_b + 1), min(n_a - 1, t)
        cur = np.full(n_a, inf, np.float32)
        i = np.arange(lo, hi + 1)
        up = np.where(i > 0, prev1[np.maximum(i - 1, 0)], inf)
        dg = np.where(i > 0, prev2[np.maximum(i - 1, 0)], inf)
        cur[lo:hi + 1] = d[i, t - i] + np.minimum(np.minimum(dg, up), prev1[i])
        prev2, prev1 = prev1, cur
    return prev1[n_a - 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--cases", default="b1,b64")
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcd_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    W = native.dtw_width()
    res = {"inner": args.inner, "reps": args.reps, "band_rows": W, "n_coef": 13, "cases": {}}
    for case in args.cases.split(","):
        if case == "b1":
            la, lb = [870], [870]
        else:
            B = int(case[1:])
            la = [int(v) for v in synth_lengths(B, 1234)[1]]
            scale = np.random.RandomState(7).uniform(0.9, 1.1, B)
            lb = [int(min(870, max(1, round(n * s)))) for n, s in zip(la, scale)]
        B = len(la)
        g = torch.Generator().manual_seed(3)
        mel_a = (-5.0 + 2.0 * torch.randn(B, 80, max(la), generator=g)).to(dev)
        mel_b = (-5.0 + 2.0 * torch.randn(B, 80, max(lb), generator=g)).to(dev)
        cost_only, with_path = audio.MelCepstralDistortion(13), audio.MelCepstralDistortion(13, return_path=True)
        ca, cb = audio.mel_cepstrum(mel_a, la, 13), audio.mel_cepstrum(mel_b, lb, 13)

        def many(fn):
            def run():
                for _ in range(args.inner):
                    fn()
            return run

        t = {"mcd_cost_only": _ms(many(lambda: cost_only(mel_a, mel_b, la, lb)), args.reps) / args.inner,
             "mcd_with_path": _ms(many(lambda: with_path(mel_a, mel_b, la, lb)), args.reps) / args.inner,
             "cepstrum_both_sides": _ms(many(lambda: (audio.mel_cepstrum(mel_a, la, 13), audio.mel_cepstrum(mel_b, lb, 13))),
                                        args.reps) / args.inner,
             "dtw_cost_only": _ms(many(lambda: audio.dtw(ca, cb, la, lb)), args.reps) / args.inner,
             "dtw_with_path": _ms(many(lambda: audio.dtw(ca, cb, la, lb, return_path=True)), args.reps) / args.inner}
        kt = kernel_times(many(lambda: with_path(mel_a, mel_b, la, lb)), ("mel_cepstrum", "dtw", "dtw_backtrack"))
        kt_cost = kernel_times(many(lambda: cost_only(mel_a, mel_b, la, lb)), ("dtw",))
        per = {k: v["ms"] / v["launches"] for k, v in kt.items()}
        per["dtw_cost_only"] = kt_cost["dtw"]["ms"] / kt_cost["dtw"]["launches"]
        steps = max(sum(nb + min(W, na - i0) - 1 for i0 in range(0, na, W)) for na, nb in zip(la, lb))
        r = {"B": B, "frames_a": [min(la), max(la)], "frames_b": [min(lb), max(lb)], "cells": int(sum(a * b for a, b in zip(la, lb))),
             "call_ms": {k: round(v, 4) for k, v in t.items()},
             "kernel_ms": {k: round(v, 4) for k, v in per.items()},
             "barrier_steps_longest_pair": steps,
             "ns_per_step_cost_only": round(per["dtw_cost_only"] * 1e6 / steps, 1),
             "ns_per_step_with_path": round(per["dtw"] * 1e6 / steps, 1)}
        if not args.no_baselines:
            native_cost = audio.dtw(ca, cb, la, lb)[0].cpu().double()
            got = torch_dtw(ca, cb, la, lb).cpu().double()
            r["torch_antidiagonal_fp32_ms"] = round(_ms(lambda: torch_dtw(ca, cb, la, lb), min(args.reps, 3)), 3)
            r["torch_max_rel_diff"] = float(((got - native_cost).abs() / native_cost).max())
            ha, hb = ca.cpu().numpy(), cb.cpu().numpy()
            t0 = time.perf_counter()
            ncost = np.array([numpy_dtw(ha[p, :la[p]], hb[p, :lb[p]]) for p in range(B)], dtype=np.float64)
            r["numpy_antidiagonal_fp32_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            r["numpy_max_rel_diff"] = float((np.abs(ncost - native_cost.numpy()) / native_cost.numpy()).max())
            r["ratio_to_torch"] = round(r["torch_antidiagonal_fp32_ms"] / t["dtw_cost_only"], 1)
            r["ratio_to_numpy"] = round(r["numpy_antidiagonal_fp32_ms"] / t["dtw_cost_only"], 1)
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
