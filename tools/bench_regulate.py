"""alignment.length_regulate and alignment.token_average on the MI355X beside two float32 torch formulations on the GPU and the
float64 numpy restatement on the CPU.  One JSON line.

    python tools/bench_regulate.py [--reps 5] [--inner 10] [--cases b1,b64,long] [--no-baselines] [--out F]

Writes the line to profiles/regulate_bench.json as well (``--out`` names another file).

Cases: ``b1`` is one utterance of 187 tokens and 870 frames at 512 channels; ``b64`` is 64 ragged utterances with the tokens and
frames of synth_lengths(64, 1234) (28 to 177 tokens, 169 to 870 frames), the frames split over the tokens by a multinomial draw
with a fixed seed; ``long`` is the adversarial one, a single token that owns 4096 frames (``tiny`` is three short utterances, for
the tests).  For each: ms per call of ``length_regulate`` with T named, forward under no_grad and forward + backward with a given
gradient, and of ``token_average`` at C = 1 with weights, the same two (a host clock around `inner` calls that end in one device
synchronise, divided by `inner`; median of `reps` after a warm-up); ms per stage, each entry between a pair of events, mean of
`inner`; the same work in float32 torch on the GPU, once as a gather through ``path`` forward and ``index_add_`` backward, once
as the loop of ``repeat_interleave`` and ``pad`` per utterance with autograd's backward; the float64 restatement on the CPU.
The outputs of the longest and the shortest utterance must agree with the restatements within the tests' tolerances; the bench
fails otherwise.  No time is a pass condition."""
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

from bench_aligner import _event_ms  # noqa: E402
from bench_mel_loss import _ms  # noqa: E402
from tacotron2_amd import alignment, native  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402
import regulate_cases as rc  # noqa: E402
import regulate_ref as rr  # noqa: E402


def _split(rng, tokens, frames):
    return 1 + rng.multinomial(frames - tokens, np.full(tokens, 1.0 / tokens))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--cases", default="b1,b64,long")
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regulate_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"inner": args.inner, "reps": args.reps, "cases": {}}
    for case in args.cases.split(","):
        rng = np.random.RandomState(1234)
        if case == "b1":
            ds, C = [_split(rng, 187, 870)], 512
        elif case == "long":
            ds, C = [np.array([4096])], 512
        elif case == "tiny":
            ds, C = [_split(rng, 9, 40), np.array([0, 3, 0, 0, 5, 1]), _split(rng, 3, 7)], 24
        else:
            ti, to = synth_lengths(int(case[1:]), 1234)
            ds, C = [_split(rng, int(n), int(t)) for n, t in zip(ti, to)], 512
        B, nl, tl = len(ds), [len(d) for d in ds], [int(d.sum()) for d in ds]
        N, T = max(nl), max(tl)
        d = torch.zeros(B, N, dtype=torch.int32)
        for b in range(B):
            d[b, :nl[b]] = torch.from_numpy(ds[b].astype(np.int32))
        gen = torch.Generator().manual_seed(3)
        x, g = torch.randn(B, N, C, generator=gen).to(dev), torch.randn(B, T, C, generator=gen).to(dev)
        v, w, gp = torch.randn(B, T, generator=gen).to(dev), torch.rand(B, T, generator=gen).to(dev), torch.randn(B, N, generator=gen).to(dev)
        d, n_dev = d.to(dev), torch.tensor(nl, dtype=torch.int32).to(dev)
        xl, vl = x.clone().requires_grad_(True), v.clone().requires_grad_(True)

        def many(fn):
            def run():
                for _ in range(args.inner):
                    fn()
            return run

        def expand():
            with torch.no_grad():
                return alignment.length_regulate(x, d, n_dev, T)[0]

        def expand_bwd():
            xl.grad = None
            alignment.length_regulate(xl, d, n_dev, T)[0].backward(g)

        def pool():
            with torch.no_grad():
                return alignment.token_average(v, d, n_dev, w)

        def pool_bwd():
            vl.grad = None
            alignment.token_average(vl, d, n_dev, w).backward(gp)

        t = {"length_regulate_forward": _ms(many(expand), args.reps) / args.inner,
             "length_regulate_forward_backward": _ms(many(expand_bwd), args.reps) / args.inner,
             "token_average_forward": _ms(many(pool), args.reps) / args.inner,
             "token_average_forward_backward": _ms(many(pool_bwd), args.reps) / args.inner}
        # ---- the stages, each entry between a pair of events
        path, t_len, ends = (torch.empty(s, dtype=torch.int32, device=dev) for s in ((B, T), (B,), (B, N)))
        y, dx = torch.empty(B, T, C, device=dev), torch.empty(B, N, C, device=dev)
        v3, m, den, dv = v.unsqueeze(2), torch.empty(B, N, 1, device=dev), torch.empty(B, N, device=dev), torch.empty(B, T, 1, device=dev)
        st = {"regulate_path_kernel": _event_ms(lambda: native.durations_to_path(d, n_dev, T, path, t_len, ends), args.inner),
              "regulate_expand_kernel": _event_ms(lambda: native.length_regulate(x, path, y), args.inner),
              "regulate_segsum_kernel": _event_ms(lambda: native.length_regulate_backward(g, ends, dx), args.inner),
              "regulate_pool_kernel": _event_ms(lambda: native.token_average(v3, w, ends, m, den), args.inner),
              "regulate_pool_bwd_kernel": _event_ms(lambda: native.token_average_backward(gp.unsqueeze(2), den, w, path, dv), args.inner)}
        r = {"B": B, "C": C, "frames": [min(tl), max(tl)], "tokens": [min(nl), max(nl)], "longest_segment": int(max(int(x_.max()) for x_ in ds)),
             "call_ms": {n: round(val, 4) for n, val in t.items()}, "kernel_ms": {n: round(val, 4) for n, val in st.items()}}
        # ---- agreement with the restatements (and the float64 one's time)
        expand_bwd()
        pool_bwd()
        torch.cuda.synchronize()
        hy, hdx, hm, hdv = expand().cpu().numpy(), xl.grad.cpu().numpy(), pool().cpu().numpy(), vl.grad.cpu().numpy()
        cx, cg, cv, cw, cgp = (a.cpu().numpy() for a in (x, g, v, w, gp))
        t0 = time.perf_counter()
        refs = []
        for b in range(B):
            p, _ = rr.path_of(ds[b], nl[b], T)
            refs.append((p, rr.expand(cx[b, :nl[b]], p), rr.segsum64(cg[b], p, nl[b]), rr.pool64(cv[b][:, None], cw[b], p, nl[b])))
        r["numpy_float64_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        worst = {"dx": 0.0, "m": 0.0, "dv": 0.0}
        for b in sorted({int(np.argmax(tl)), int(np.argmin(tl))}):
            p, y_ref, (dx64, mag, cnt), p64 = refs[b]
            n = nl[b]
            if not np.array_equal(rc.bits(hy[b]), rc.bits(y_ref)) or not np.array_equal(rc.bits(hdx[b, :n]), rc.bits(rr.segsum32(cg[b], p, n))):
                raise SystemExit("bench_regulate: y or dx differ from the float32 restatement (%s, utterance %d)" % (case, b))
            p32 = rr.pool32(cv[b][:, None], cw[b], p, n)
            dv32 = rr.pool_bwd(cgp[b, :n, None], p32["den"], cw[b], p, np.float32)
            if rr.ulps(hm[b, :n], p32["m"][:, 0]).max() > rc.MAX_ULPS or rr.ulps(hdv[b], dv32[:, 0]).max() > rc.MAX_ULPS:
                raise SystemExit("bench_regulate: m or dv differ from the float32 restatement (%s, utterance %d)" % (case, b))
            allow = rr.gamma(cnt - 1)[:, None] * mag
            worst["dx"] = max(worst["dx"], float((np.abs(hdx[b, :n] - dx64) / np.where(allow > 0, allow, 1.0)).max()))
            allow = rr.pool_allowed(p64)
            worst["m"] = max(worst["m"], float((np.abs(hm[b, :n, None] - p64["m"]) / np.where(allow > 0, allow, 1.0)).max()))
            dv64 = rr.pool_bwd(cgp[b, :n, None], p64["den"], cw[b], p, np.float64)
            allow = 2.0 * np.abs(dv64) * (rr.gamma(np.where(p >= 0, cnt[np.maximum(p, 0)], 1) - 1) + 2 * rr.U)[:, None]
            worst["dv"] = max(worst["dv"], float((np.abs(hdv[b][:, None] - dv64) / np.where(allow > 0, allow, 1.0)).max()))
        r["error_over_allowed"] = {n: round(val, 4) for n, val in worst.items()}
        if max(worst.values()) > 1.0:
            raise SystemExit("bench_regulate: disagrees with the float64 restatement (%s, %s of the allowed error)" % (case, worst))
        r["ratio_to_numpy"] = round(r["numpy_float64_ms"] / (t["length_regulate_forward_backward"] + t["token_average_forward_backward"]), 1)
        if not args.no_baselines:
            tx = x.clone().requires_grad_(True)
            hp = torch.from_numpy(np.stack([q[0] for q in refs]).astype(np.int64)).to(dev)
            live, idx = (hp >= 0), hp.clamp_min(0)
            flat = (idx + N * torch.arange(B, device=dev)[:, None]).reshape(-1)

            def gather():                                                   # forward a gather through path, backward index_add_
                yy = torch.gather(x, 1, idx[:, :, None].expand(B, T, C)) * live[:, :, None]
                dd = torch.zeros(B * N, C, device=dev).index_add_(0, flat, (g * live[:, :, None]).reshape(B * T, C))
                return yy, dd

            def loop():                                                     # the per-utterance repeat_interleave + pad loop, autograd
                tx.grad = None
                rows = [torch.nn.functional.pad(torch.repeat_interleave(tx[b, :nl[b]], d[b, :nl[b]].long(), dim=0, output_size=tl[b]),
                                                (0, 0, 0, T - tl[b])) for b in range(B)]
                torch.stack(rows).backward(g)

            r["torch_float32_gather_index_add_ms"] = round(_ms(many(gather), args.reps) / args.inner, 4)
            r["torch_float32_repeat_interleave_loop_ms"] = round(_ms(many(loop), args.reps) / args.inner, 4)
            yy, dd = gather()
            r["torch_gather_equals_y_bit_for_bit"] = bool(torch.equal(yy, expand()))
            r["torch_index_add_max_abs_difference_of_dx"] = float((dd.view(B, N, C) - xl.grad).abs().max())
            r["ratio_to_torch_gather_index_add"] = round(r["torch_float32_gather_index_add_ms"] / t["length_regulate_forward_backward"], 2)
            r["ratio_to_torch_repeat_interleave_loop"] = round(r["torch_float32_repeat_interleave_loop_ms"] / t["length_regulate_forward_backward"], 2)
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
