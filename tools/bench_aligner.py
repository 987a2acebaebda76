"""alignment.aligner_scores on the MI355X beside the float32 torch formulation on the GPU and the float64 numpy restatement on the
CPU.  One JSON line.

    python tools/bench_aligner.py [--reps 5] [--inner 10] [--cases b1,b64] [--no-baselines] [--out F]

Writes the line to profiles/aligner_bench.json as well (``--out`` names another file).

Cases: B = 1 at 870 frames x 187 tokens x 80 channels, and B = 64 ragged with the tokens and frames of synth_lengths(64, 1234)
(``tiny`` is three short utterances, for the tests).  Queries and keys are randn, the prior is the beta-binomial one of scaling 1,
the temperature 0.0005.  For each: ms per call of ``aligner_scores`` under no_grad (forward alone), of forward + backward with a
given gradient, and of forward + backward through ``ForwardSumLoss`` (a host clock around `inner` calls that end in one device
synchronise, divided by `inner`; median of `reps` after a warm-up); ms per stage, each between a pair of events, mean of `inner`:
the packing kernel, the forward row pass, the backward row pass with its column sums (one entry), the two transposes and each of
the three products from launches of their own entries, beside the whole forward and the whole backward; the same forward + backward in float32 torch on the GPU (the
broadcast difference where its (B, T, N, C) tensor stays below 2 GiB, else cdist squared); the float64 restatement on the CPU.
The scores and both gradients of the longest and the shortest utterance must agree with the restatement within the tests'
tolerance; the bench fails otherwise.  No time is a pass condition."""
import argparse
import ctypes
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

from bench_mel_loss import _ms  # noqa: E402
from tacotron2_amd import alignment, native  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402
import aligner_ref as ar  # noqa: E402

TAU = 0.0005


def _event_ms(fn, inner):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--cases", default="b1,b64")
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aligner_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = native.load()
    res = {"inner": args.inner, "reps": args.reps, "temperature": TAU, "cases": {}}
    for case in args.cases.split(","):
        if case == "b1":
            nl, tl, C = [187], [870], 80
        elif case == "tiny":
            nl, tl, C = [9, 20, 3], [40, 33, 7], 24
        else:
            ti, to = synth_lengths(int(case[1:]), 1234)
            nl, tl, C = [int(v) for v in ti], [int(v) for v in to], 80
        B, Tm, Nm = len(tl), max(tl), max(nl)
        gen = torch.Generator().manual_seed(3)
        q, k = torch.randn(B, Tm, C, generator=gen).to(dev), torch.randn(B, Nm, C, generator=gen).to(dev)
        g = torch.randn(B, Tm, Nm, generator=gen).to(dev)
        lp = alignment.beta_binomial_log_prior(tl, nl, 1.0, Tm, Nm, dev)
        ql, kl = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
        loss = alignment.ForwardSumLoss()

        def many(fn):
            def run():
                for _ in range(args.inner):
                    fn()
            return run

        def fwd():
            with torch.no_grad():
                return alignment.aligner_scores(q, k, tl, nl, TAU, lp)

        def fwd_bwd():
            ql.grad = kl.grad = None
            alignment.aligner_scores(ql, kl, tl, nl, TAU, lp).backward(g)

        def fwd_bwd_loss():
            ql.grad = kl.grad = None
            loss(alignment.aligner_scores(ql, kl, tl, nl, TAU, lp), tl, nl).backward()

        t = {"forward": _ms(many(fwd), args.reps) / args.inner, "forward_backward": _ms(many(fwd_bwd), args.reps) / args.inner,
             "forward_backward_loss": _ms(many(fwd_bwd_loss), args.reps) / args.inner}
        # ---- the stages, each between a pair of events
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())   # noqa: E731
        t_dev, n_dev = (torch.tensor(v, dtype=torch.int32).to(dev) for v in (tl, nl))
        s = torch.empty(B, Tm, Nm, device=dev)
        kept = torch.empty(native.aligner_workspace(B, Tm, Nm, C, 1), dtype=torch.uint8, device=dev)
        ws = torch.empty(native.aligner_workspace(B, Tm, Nm, C, 2), dtype=torch.uint8, device=dev)
        dq, dk = torch.empty_like(q), torch.empty_like(k)
        Np, Cp = (Nm + 31) // 32 * 32, (C + 31) // 32 * 32
        Kp, kn = torch.empty(B, Nm, Cp, device=dev), torch.empty(B, Nm, device=dev)
        lse, dz, cs = torch.empty(B, Tm, device=dev), torch.zeros(B, Tm, Np, device=dev), torch.empty(B, Nm, device=dev)
        KT, QT = torch.empty(B, C, Np, device=dev), torch.empty(B, C, (Tm + 31) // 32 * 32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        st = {}
        st["full_forward"] = _event_ms(lambda: native.aligner_scores(q, k, t_dev, n_dev, TAU, lp, s, kept, True), args.inner)
        st["full_backward"] = _event_ms(lambda: native.aligner_scores_backward(q, k, t_dev, n_dev, TAU, g, dq, dk, None, kept, ws), args.inner)
        st["aligner_pack_keys_kernel"] = _event_ms(lambda: lib.t2amd_aligner_pack_keys_f32(p(k), p(n_dev), B, Nm, C, p(Kp), p(kn), stream), args.inner)
        z0 = s.clone()
        st["aligner_rows_fwd_kernel"] = _event_ms(lambda: lib.t2amd_aligner_rows_fwd_f32(p(z0), Tm * Nm, Nm, p(lp), Tm * Nm, Nm, p(t_dev), p(n_dev),
                                                                                       B, Tm, Nm, p(lse), stream), args.inner)
        st["aligner_rows_bwd_kernel+aligner_colsum_kernel"] = _event_ms(
            lambda: lib.t2amd_aligner_rows_bwd_f32(p(g), Tm * Nm, Nm, p(t_dev), p(n_dev), B, Tm, Nm, p(lse), p(dz), p(cs), None, 0, 0, stream), args.inner)
        st["aligner_transpose_kernel x2"] = _event_ms(lambda: (lib.t2amd_aligner_transpose_f32(p(k), p(n_dev), B, Nm, C, p(KT), stream),
                                                              lib.t2amd_aligner_transpose_f32(p(q), p(t_dev), B, Tm, C, p(QT), stream)), args.inner)
        # the three products on the slabs the whole backward left in ws (z leaves z in the dz slab: it runs last)
        prod = lambda which: lib.t2amd_aligner_product_f32(which, p(q), p(k), p(t_dev), p(n_dev), B, Tm, Nm, C, TAU, p(dq), p(dk),   # noqa: E731
                                                           p(kept), kept.numel(), p(ws), ws.numel(), stream)
        native.aligner_scores_backward(q, k, t_dev, n_dev, TAU, g, dq, dk, None, kept, ws)
        st["aligner_dq_kernel"] = _event_ms(lambda: prod(2), args.inner)
        st["aligner_dk_kernel"] = _event_ms(lambda: prod(3), args.inner)
        st["aligner_z_kernel"] = _event_ms(lambda: prod(1), args.inner)
        r = {"B": B, "C": C, "frames": [min(tl), max(tl)], "tokens": [min(nl), max(nl)], "cells": int(sum(a * b for a, b in zip(tl, nl))),
             "call_ms": {n: round(v, 4) for n, v in t.items()}, "kernel_ms": {n: round(v, 4) for n, v in st.items()}}
        # ---- agreement with the float64 restatement (and its time)
        fwd_bwd()
        torch.cuda.synchronize()
        hs, hq, hk = fwd().cpu().numpy(), ql.grad.cpu().numpy(), kl.grad.cpu().numpy()
        cq, ck, cg, cl = q.cpu().numpy(), k.cpu().numpy(), g.cpu().numpy(), lp.cpu().numpy()
        t0 = time.perf_counter()
        refs = []
        for b in range(B):
            T, N = tl[b], nl[b]
            refs.append((ar.scores64(cq[b, :T], ck[b, :N], TAU, cl[b, :T, :N])["s"], ar.grads64(cq[b, :T], ck[b, :N], TAU, cg[b, :T, :N])))
        r["numpy_float64_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        worst = {"s": 0.0, "dq": 0.0, "dk": 0.0}
        for b in sorted({int(np.argmax(tl)), int(np.argmin(tl))}):
            T, N = tl[b], nl[b]
            s32 = ar.scores32(cq[b, :T], ck[b, :N], TAU, cl[b, :T, :N])["s"]
            own = ar.grads32(cq[b, :T], ck[b, :N], TAU, cg[b, :T, :N])
            for name, got, v32, v64 in (("s", hs[b, :T, :N], s32, refs[b][0]), ("dq", hq[b, :T], own[0], refs[b][1][0]),
                                        ("dk", hk[b, :N], own[1], refs[b][1][1])):
                worst[name] = max(worst[name], ar.error(got, v64) / ar.allowed(v32, v64))
        r["error_over_allowed"] = {n: round(v, 4) for n, v in worst.items()}
        if max(worst.values()) > 1.0:
            raise SystemExit("bench_aligner: disagrees with the float64 restatement (%s, %s of the allowed error)" % (case, worst))
        r["ratio_to_numpy"] = round(r["numpy_float64_ms"] / t["forward_backward"], 1)
        if not args.no_baselines:
            broadcast = 4 * B * Tm * Nm * C < 2 ** 31
            tq, tk = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
            mask = torch.zeros(B, Tm, Nm, dtype=torch.bool, device=dev)
            for b in range(B):
                mask[b, :tl[b], :nl[b]] = True
            gm = torch.where(mask, g, torch.zeros_like(g))
            nmask = mask.any(dim=1, keepdim=True)

            def torch32():
                tq.grad = tk.grad = None
                d = ((tq[:, :, None, :] - tk[:, None, :, :]) ** 2).sum(dim=3) if broadcast else torch.cdist(tq, tk) ** 2
                z = torch.where(nmask, -TAU * d, torch.full_like(d, float("-inf")))          # a padded frame keeps its tokens
                sc = torch.log_softmax(z, dim=2) + torch.where(mask, lp, torch.zeros_like(lp))
                torch.where(mask, sc, torch.zeros_like(sc)).backward(gm)
                return sc

            r["torch_float32_formulation"] = "broadcast difference" if broadcast else "cdist squared"
            r["torch_float32_forward_backward_ms"] = round(_ms(many(torch32), args.reps) / args.inner, 4)
            sc = torch32().detach()
            r["torch_float32_max_abs_difference_of_scores"] = float((torch.where(mask, sc, torch.zeros_like(sc)).cpu()
                                                                     - torch.from_numpy(np.where(np.isfinite(hs), hs, 0.0))).abs().max())
            r["ratio_to_torch_float32"] = round(r["torch_float32_forward_backward_ms"] / t["forward_backward"], 2)
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
