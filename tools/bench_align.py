"""alignment.monotonic_align on the MI355X beside two statements of the same recurrence, one frame at a time: float32 torch ops on
the GPU and a float32 numpy loop on the CPU.  One JSON line.

    python tools/bench_align.py [--reps 5] [--inner 10] [--cases b1,b64] [--no-baselines] [--out F]

Writes the line to profiles/align_bench.json as well (``--out`` names another file).

Cases: B = 1 at 870 frames x 187 tokens, and B = 64 ragged with the tokens and frames of synth_lengths(64, 1234).  The scores are
log-softmax rows of 2 randn.  For each: ms per call of ``alignment.monotonic_align`` without and with the path (a host clock
around `inner` calls that end in one device synchronise, divided by `inner`; median of `reps` after a warm-up); ms per launch of
the kernel (each launch between a pair of events, mean of `inner`); the kernel's own two clock counts (100 MHz) of the utterance
with the most frames: the recurrence and the backtrack, and the recurrence's ns per frame; the torch statement (pad / gt / where /
add per frame, the whole batch per op, the choices kept, then the walk on the host) and the numpy statement (the same per
utterance).  Both baselines must give the native score bit for bit and the native durations; the bench fails otherwise.
ratio_* is the baseline's time over the native call without the path (above 1: the native path is faster)."""
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
from tacotron2_amd import alignment, native  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402


def walk(adv, T, N):
    """Durations from the choices ``adv`` (T, N) bool: from (T-1, N-1), n = 0 stays and n = t advances whatever is stored."""
    dur = np.zeros(N, dtype=np.int32)
    n = N - 1
    for t in range(T - 1, 0, -1):
        dur[n] += 1
        if n > 0 and (n == t or adv[t, n]):
            n -= 1
    dur[n] += 1
    return dur


def torch_recurrence(x):
    """Q (T, B, N) float32 and the choices (T, B, N) bool of the recurrence as torch ops, one set per frame, the batch per op."""
    B, T, N = x.shape
    ninf = float("-inf")
    Q = torch.empty(T, B, N, device=x.device)
    adv = torch.zeros(T, B, N, dtype=torch.bool, device=x.device)
    Q[0] = ninf
    Q[0, :, 0] = x[:, 0, 0]
    pad = torch.nn.functional.pad
    for t in range(1, T):
        stay = Q[t - 1]
        move = pad(stay[:, :-1], (1, 0), value=ninf)
        torch.gt(move, stay, out=adv[t])
        torch.add(x[:, t], torch.where(adv[t], move, stay), out=Q[t])
    return Q, adv


def numpy_align(x):
    """(score, durations) of one (T, N) float32 matrix as a numpy loop over frames."""
    T, N = x.shape
    ninf = np.float32(-np.inf)
    q = np.full(N, ninf, np.float32)
    q[0] = x[0, 0]
    adv = np.zeros((T, N), dtype=bool)
    for t in range(1, T):
        move = np.concatenate([[ninf], q[:-1]]).astype(np.float32)
        adv[t] = move > q
        q = x[t] + np.where(adv[t], move, q)
    return q[N - 1], walk(adv, T, N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--cases", default="b1,b64")
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    W, max_t, max_n = native.align_limits()
    res = {"inner": args.inner, "reps": args.reps, "lanes": W, "max_frames": max_t, "max_tokens": max_n, "cases": {}}
    for case in args.cases.split(","):
        if case == "b1":
            nl, tl = [187], [870]
        else:
            ti, to = synth_lengths(int(case[1:]), 1234)
            nl, tl = [int(v) for v in ti], [int(v) for v in to]
        B, Tm, Nm = len(tl), max(tl), max(nl)
        g = torch.Generator().manual_seed(3)
        x = torch.log_softmax(2.0 * torch.randn(B, Tm, Nm, generator=g), dim=2).to(dev)

        def many(fn):
            def run():
                for _ in range(args.inner):
                    fn()
            return run

        t = {"without_path": _ms(many(lambda: alignment.monotonic_align(x, tl, nl)), args.reps) / args.inner,
             "with_path": _ms(many(lambda: alignment.monotonic_align(x, tl, nl, return_path=True)), args.reps) / args.inner}
        per = {}
        for key, wp in (("without_path", False), ("with_path", True)):
            kt = kernel_times(many(lambda: alignment.monotonic_align(x, tl, nl, return_path=wp)), ("monotonic_align",))
            per[key] = kt["monotonic_align"]["ms"] / kt["monotonic_align"]["launches"]
        # the kernel's own clock counts, from a launch on a workspace the bench keeps
        t_dev, n_dev = (torch.tensor(v, dtype=torch.int32).to(dev) for v in (tl, nl))
        dur = torch.empty(B, Nm, dtype=torch.int32, device=dev)
        score = torch.empty(B, device=dev)
        ws = torch.zeros(native.align_workspace(B, Tm, Nm), dtype=torch.uint8, device=dev)
        native.monotonic_align(x, t_dev, n_dev, dur, score, None, ws)
        native.monotonic_align(x, t_dev, n_dev, dur, score, None, ws)
        torch.cuda.synchronize()
        ticks = ws[-16 * B:].cpu().numpy().view(np.uint64).reshape(B, 2)
        lb = int(np.argmax(tl))
        r = {"B": B, "frames": [min(tl), max(tl)], "tokens": [min(nl), max(nl)], "cells": int(sum(a * b for a, b in zip(tl, nl))),
             "columns_per_lane": 1 if Nm <= W else 4,
             "call_ms": {k: round(v, 4) for k, v in t.items()},
             "kernel_ms": {k: round(v, 4) for k, v in per.items()},
             "longest_utterance": {"frames": tl[lb], "tokens": nl[lb], "recurrence_us": float(ticks[lb, 0]) / 100.0,
                                   "backtrack_us": float(ticks[lb, 1]) / 100.0,
                                   "ns_per_frame": round(float(ticks[lb, 0]) * 10.0 / max(1, tl[lb] - 1), 1)},
             "backtrack_us_max_over_batch": float(ticks[:, 1].max()) / 100.0}
        if not args.no_baselines:
            hs, hd = score.cpu().numpy(), dur.cpu().numpy()

            def torch_call():
                Q, adv = torch_recurrence(x)
                return Q, adv

            r["torch_per_frame_recurrence_ms"] = round(_ms(torch_call, min(args.reps, 3)), 3)
            t0 = time.perf_counter()
            Q, adv = torch_recurrence(x)
            tq = Q[t_dev.long() - 1, torch.arange(B, device=dev), n_dev.long() - 1].cpu().numpy()
            hadv = adv.cpu().numpy()
            tdur = np.zeros_like(hd)
            for b in range(B):
                tdur[b, :nl[b]] = walk(hadv[:tl[b], b, :nl[b]], tl[b], nl[b])
            r["torch_per_frame_with_host_walk_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            if not (np.array_equal(tq.view(np.int32), hs.view(np.int32)) and np.array_equal(tdur, hd)):
                raise SystemExit("bench_align: the torch statement disagrees with the native result (%s)" % case)
            hx = x.cpu().numpy()
            t0 = time.perf_counter()
            got = [numpy_align(hx[b, :tl[b], :nl[b]]) for b in range(B)]
            r["numpy_per_frame_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            for b, (s, d) in enumerate(got):
                if np.float32(s).view(np.int32) != hs.view(np.int32)[b] or not np.array_equal(d, hd[b, :nl[b]]):
                    raise SystemExit("bench_align: the numpy statement disagrees with the native result (%s, %d)" % (case, b))
            r["baselines_agree_exactly"] = True
            r["ratio_to_torch_recurrence"] = round(r["torch_per_frame_recurrence_ms"] / t["without_path"], 1)
            r["ratio_to_torch_with_walk"] = round(r["torch_per_frame_with_host_walk_ms"] / t["without_path"], 1)
            r["ratio_to_numpy"] = round(r["numpy_per_frame_ms"] / t["without_path"], 1)
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
