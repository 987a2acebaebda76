"""transformer.self_attention on the MI355X beside two float32 torch baselines on the same inputs.  One JSON line.

    python tools/bench_self_attn.py [--reps 5] [--inner 10] [--cases b1,b16,b16wide,b64] [--no-baselines] [--out F]

Writes the line to profiles/self_attn_bench.json as well (``--out`` names another file).

Cases: ``b1`` is one utterance of 870 frames at H = 1, D = 64; ``b16`` is 16 ragged utterances with the frames of
synth_lengths(16, 1234) (147 to 859) at H = 1, D = 64 and ``b16wide`` the same at H = 2, D = 128; ``b64`` is 64 ragged utterances
at the token rate (the tokens of synth_lengths(64, 1234), 28 to 177) at H = 2, D = 64 (``tiny`` is three short utterances, for the
tests).  q, k and v are the chunks of one packed projection.  For each: ms per call of the forward under no_grad and of forward +
backward with a given gradient (a host clock around `inner` calls that end in one device synchronise, divided by `inner`; median
of `reps` after a warm-up); ms per kernel, each entry between a pair of events, mean of `inner`; the same for the float32 torch
formulation (bmm / masked_fill / softmax / bmm with autograd) and for F.scaled_dot_product_attention with a boolean mask; and
torch.cuda.max_memory_allocated over one forward + backward of each, above what was allocated before it.  The longest and the
shortest utterance must agree with the float64 restatement within the tests' tolerance; the bench fails otherwise.  No time is a
pass condition."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_aligner import _event_ms  # noqa: E402
from bench_mel_loss import _ms  # noqa: E402
from tacotron2_amd import native, transformer  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402
import self_attn_ref as sr  # noqa: E402


def _peak(fn):
    """Bytes fn() allocates at its peak above what is allocated now."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--cases", default="b1,b16,b16wide,b64")
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_attn_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"inner": args.inner, "reps": args.reps, "cases": {}}
    for case in args.cases.split(","):
        if case == "b1":
            tl, H, D = [870], 1, 64
        elif case == "b16":
            tl, H, D = [int(t) for t in synth_lengths(16, 1234)[1]], 1, 64
        elif case == "b16wide":
            tl, H, D = [int(t) for t in synth_lengths(16, 1234)[1]], 2, 128
        elif case == "b64":
            tl, H, D = [int(t) for t in synth_lengths(64, 1234)[0]], 2, 64
        elif case == "tiny":
            tl, H, D = [40, 3, 70], 2, 32
        else:
            raise SystemExit("bench_self_attn: unknown case %r" % case)
        B, T = len(tl), max(tl)
        gen = torch.Generator().manual_seed(3)
        qkv = torch.randn(B, T, 3 * H * D, generator=gen).to(dev)
        g = torch.randn(B, T, H, D, generator=gen).to(dev)
        lens = torch.tensor(tl, dtype=torch.int32).to(dev)
        scale = float(D) ** -0.5
        leaf = qkv.clone().requires_grad_(True)
        chunks = lambda x: [c.view(B, T, H, D) for c in x.chunk(3, dim=2)]      # noqa: E731

        def many(fn):
            def run():
                for _ in range(args.inner):
                    fn()
            return run

        def fwd():
            with torch.no_grad():
                return transformer.self_attention(*chunks(qkv), lens)

        def fwd_bwd():
            leaf.grad = None
            transformer.self_attention(*chunks(leaf), lens).backward(g)

        t = {"forward": _ms(many(fwd), args.reps) / args.inner, "forward_backward": _ms(many(fwd_bwd), args.reps) / args.inner}
        q, k, v = chunks(qkv)
        o, dq, dk, dv = (torch.empty(B, T, H, D, device=dev) for _ in range(4))
        lse = torch.empty(B, H, T, device=dev)
        ws = torch.empty(native.self_attn_workspace(B, T, H, D, 2), dtype=torch.uint8, device=dev)
        st = {"self_attn_fwd_kernel": _event_ms(lambda: native.self_attn(q, k, v, lens, scale, o, lse), args.inner),
              "self_attn_delta_kernel": _event_ms(lambda: native.self_attn_delta(g, o, lens, ws.view(torch.float32)[:B * H * T].view(B, H, T)),
                                                  args.inner),
              "self_attn_backward_three_kernels": _event_ms(lambda: native.self_attn_backward(q, k, v, o, lse, g, lens, scale, dq, dk, dv, ws),
                                                            args.inner)}
        r = {"B": B, "H": H, "D": D, "frames": [min(tl), max(tl)], "call_ms": {n: round(val, 4) for n, val in t.items()},
             "kernel_ms": {n: round(val, 4) for n, val in st.items()},
             "peak_bytes": {"forward_no_grad": _peak(fwd), "forward_backward": _peak(fwd_bwd)},
             "one_score_matrix_bytes": 4 * B * H * T * T}
        # ---- agreement with the float64 restatement, the longest and the shortest utterance
        fwd_bwd()
        torch.cuda.synchronize()
        ho, hg = fwd().cpu().numpy(), leaf.grad.cpu().numpy()
        cq, ck, cv = (c.cpu().numpy() for c in chunks(qkv))
        hd = [c for c in np.split(hg, 3, axis=2)]
        worst = {}
        for b in sorted({int(np.argmax(tl)), int(np.argmin(tl))}):
            n = tl[b]
            a = (cq[b, :n], ck[b, :n], cv[b, :n], g[b, :n].cpu().numpy())
            f64, f32 = sr.attention64(*a, scale), sr.attention32(*a, scale)
            got = {"o": ho[b, :n], "dq": hd[0][b, :n].reshape(n, H, D), "dk": hd[1][b, :n].reshape(n, H, D), "dv": hd[2][b, :n].reshape(n, H, D)}
            for name, x in got.items():
                worst[name] = max(worst.get(name, 0.0), sr.error(x, f64[name]) / sr.allowed(f32[name], f64[name]))
            if ho[b, n:].any() or hg[b, n:].any():
                raise SystemExit("bench_self_attn: the padding of utterance %d is not zero (%s)" % (b, case))
        r["error_over_allowed"] = {n: round(val, 4) for n, val in worst.items()}
        if max(worst.values()) > 1.0:
            raise SystemExit("bench_self_attn: disagrees with the float64 restatement (%s, %s of the allowed error)" % (case, worst))
        if not args.no_baselines:
            dead = (torch.arange(T, device=dev)[None, :] >= lens[:, None])                      # (B, T)
            tleaf = qkv.clone().requires_grad_(True)

            def heads(x):
                return [c.view(B, T, H, D).permute(0, 2, 1, 3) for c in x.chunk(3, dim=2)]     # (B, H, T, D)

            def formulation():
                tleaf.grad = None
                tq, tk, tv = (c.reshape(B * H, T, D) for c in heads(tleaf))
                s = torch.bmm(tq, tk.transpose(1, 2)).mul_(scale).view(B, H, T, T).masked_fill(dead[:, None, None, :], float("-inf"))
                to = torch.bmm(torch.softmax(s, dim=3).view(B * H, T, T), tv).view(B, H, T, D).permute(0, 2, 1, 3)
                to.backward(g)
                return to

            def sdpa():
                tleaf.grad = None
                tq, tk, tv = heads(tleaf)
                to = torch.nn.functional.scaled_dot_product_attention(tq, tk, tv, attn_mask=~dead[:, None, None, :], scale=scale)
                to = to.permute(0, 2, 1, 3)
                to.backward(g)
                return to

            for name, fn in (("torch_float32_bmm_softmax_bmm", formulation), ("torch_scaled_dot_product_attention", sdpa)):
                r[name] = {"forward_backward_ms": round(_ms(many(fn), args.reps) / args.inner, 4), "peak_bytes": _peak(fn)}
                live = (~dead)[:, :, None, None]
                r[name]["max_abs_difference_of_o"] = float(((fn().detach() - fwd()) * live).abs().max())
                r[name]["ratio_to_native"] = round(r[name]["forward_backward_ms"] / t["forward_backward"], 2)
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
