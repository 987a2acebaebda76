"""alignment.forward_sum on the MI355X beside F.ctc_loss on the GPU (a blank column of -inf, forward + backward) and the float64
numpy restatement on the CPU.  One JSON line.

    python tools/bench_forward_sum.py [--reps 5] [--inner 10] [--cases b1,b64] [--no-baselines] [--out F]

Writes the line to profiles/forward_sum_bench.json as well (``--out`` names another file).

Cases: B = 1 at 870 frames x 187 tokens, and B = 64 ragged with the tokens and frames of synth_lengths(64, 1234).  The scores are
log-softmax rows of 2 randn.  For each: ms per call of ``alignment.forward_sum`` under no_grad (forward alone) and of forward +
``.sum().backward()`` (a host clock around `inner` calls that end in one device synchronise, divided by `inner`; median of `reps`
after a warm-up); ms per launch of the two kernels (each launch between a pair of events, mean of `inner`); the kernels' own clock
counts (100 MHz) of the utterance with the most frames, alpha and beta, and their ns per frame; ``F.ctc_loss`` forward + backward
on the GPU in float32; the float64 restatement per utterance on the CPU.  log Z must agree with the restatement within the
tests' tolerance (8 2^-24 max(1, |log Z|), or 4 x the float32 restatement's own error where that is larger); the bench fails
otherwise.  ratio_* is the baseline's time over the native forward + backward (above 1: the native path is faster)."""
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
from tacotron2_amd import alignment, native  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402
import forward_sum_ref as fr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--cases", default="b1,b64")
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_sum_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"inner": args.inner, "reps": args.reps, "cases": {}}
    for case in args.cases.split(","):
        if case == "b1":
            nl, tl = [187], [870]
        else:
            ti, to = synth_lengths(int(case[1:]), 1234)
            nl, tl = [int(v) for v in ti], [int(v) for v in to]
        B, Tm, Nm = len(tl), max(tl), max(nl)
        g = torch.Generator().manual_seed(3)
        x = torch.log_softmax(2.0 * torch.randn(B, Tm, Nm, generator=g), dim=2).to(dev)
        leaf = x.clone().requires_grad_(True)

        def many(fn):
            def run():
                for _ in range(args.inner):
                    fn()
            return run

        def fwd():
            with torch.no_grad():
                return alignment.forward_sum(x, tl, nl)

        def fwd_bwd():
            leaf.grad = None
            alignment.forward_sum(leaf, tl, nl).sum().backward()

        t = {"forward": _ms(many(fwd), args.reps) / args.inner, "forward_backward": _ms(many(fwd_bwd), args.reps) / args.inner}
        kt = kernel_times(many(fwd_bwd), ("forward_sum", "forward_sum_backward"))
        per = {k: kt[k]["ms"] / kt[k]["launches"] for k in kt}
        # the kernels' own clock counts, from launches on a workspace the bench keeps
        t_dev, n_dev = (torch.tensor(v, dtype=torch.int32).to(dev) for v in (tl, nl))
        z = torch.empty(B, device=dev)
        grad = torch.empty(B, Tm, Nm, device=dev)
        ws = torch.zeros(native.forward_sum_workspace(B, Tm, Nm, True), dtype=torch.uint8, device=dev)
        for _ in range(2):
            native.forward_sum(x, t_dev, n_dev, z, ws, True)
            native.forward_sum_backward(x, t_dev, n_dev, z, None, grad, None, ws)
        torch.cuda.synchronize()
        ticks = ws[-16 * B:].cpu().numpy().view(np.uint64).reshape(B, 2)
        lb = int(np.argmax(tl))
        r = {"B": B, "frames": [min(tl), max(tl)], "tokens": [min(nl), max(nl)], "cells": int(sum(a * b for a, b in zip(tl, nl))),
             "columns_per_lane": 1 if Nm <= 256 else 4,
             "call_ms": {k: round(v, 4) for k, v in t.items()},
             "kernel_ms": {k: round(v, 4) for k, v in per.items()},
             "longest_utterance": {"frames": tl[lb], "tokens": nl[lb], "alpha_us": float(ticks[lb, 0]) / 100.0,
                                   "beta_us": float(ticks[lb, 1]) / 100.0,
                                   "alpha_ns_per_frame": round(float(ticks[lb, 0]) * 10.0 / tl[lb], 1),
                                   "beta_ns_per_frame": round(float(ticks[lb, 1]) * 10.0 / tl[lb], 1)}}
        hx, hz = x.cpu().numpy(), z.cpu().numpy()
        t0 = time.perf_counter()
        refs = [fr.forward_sum64(hx[b, :tl[b], :nl[b]]) for b in range(B)]
        r["numpy_float64_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        worst = 0.0
        for b in (range(B) if B <= 4 else [lb, int(np.argmin(tl))]):
            z32 = fr.forward_sum32(hx[b, :tl[b], :nl[b]])[0]
            tol = max(4 * abs(float(z32) - refs[b][0]), 8 * fr.U * max(1.0, abs(refs[b][0])))
            worst = max(worst, abs(float(hz[b]) - refs[b][0]) / tol)
        r["log_z_error_over_allowed"] = round(worst, 4)
        if worst > 1.0:
            raise SystemExit("bench_forward_sum: log Z disagrees with the float64 restatement (%s, %.3f of the allowed error)"
                             % (case, worst))
        r["ratio_to_numpy"] = round(r["numpy_float64_ms"] / t["forward_backward"], 1)
        if not args.no_baselines:
            tgt = torch.zeros(B, Nm, dtype=torch.long)
            for b in range(B):
                tgt[b, :nl[b]] = torch.arange(1, nl[b] + 1)
            tgt, il, ol = tgt.to(dev), torch.tensor(tl), torch.tensor(nl)
            cleaf = x.clone().requires_grad_(True)

            def ctc():
                cleaf.grad = None
                lp = torch.cat([torch.full((B, Tm, 1), float("-inf"), device=dev), cleaf], dim=2).transpose(0, 1)
                loss = torch.nn.functional.ctc_loss(lp, tgt, il, ol, blank=0, reduction='none')
                loss.sum().backward()
                return loss

            r["ctc_loss_forward_backward_ms"] = round(_ms(many(ctc), args.reps) / args.inner, 4)
            r["ctc_loss_max_abs_difference_of_log_z"] = float((ctc().detach().cpu() + z.cpu()).abs().max())
            r["ratio_to_ctc_loss"] = round(r["ctc_loss_forward_backward_ms"] / t["forward_backward"], 2)
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
