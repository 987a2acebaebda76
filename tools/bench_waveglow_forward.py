"""WaveGlow's forward direction (audio -> latents, WaveGlow.forward) on the MI355X: one JSON line.

    python tools/bench_waveglow_forward.py [--reps 3] [--cases b1,b16,train] [--precisions fp32,bf16x3,bf16]
                                           [--no-baseline] [--out profiles/waveglow_forward_bench.json]

Model: the published geometry (80 mels, 12 flows, n_group 8, early outputs of 2 every 4 flows, WN 8 layers of 256
channels) with tests/waveglow_ref.py's seeded weights.  Cases: B = 1 at 870 frames and B = 16 ragged
(synth_lengths(16, 1234)), the two cases of tools/bench_waveglow.py, and B = 12 segments of 16000 samples with 63 mel
frames (NVIDIA's training batch).  For each case and precision: ms per ``forward`` call and per ``infer`` call at the same
shape in the same run (median of `reps` after one warm-up), their ratio, ms per ``nll`` call, and the relative L2 of z
against the fp32 mode.  Baseline: the float32 restatement tests/waveglow_fwd_ref.py (eager torch, weight norm included)
on the same GPU, on the padded batch.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import waveglow_fwd_ref as fr  # noqa: E402
import waveglow_ref as wr  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402
from tacotron2_amd.waveglow import WaveGlow  # noqa: E402


def _ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="b1,b16,train")
    ap.add_argument("--precisions", default="fp32,bf16x3,bf16")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "waveglow_forward_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    C, L = 256, 8
    ref = wr.make_ref(C=C, L=L, seed=0)
    wg = WaveGlow.from_module(ref).to(dev).eval()
    ref = ref.to(dev)
    res = {"model": dict(C=C, L=L, n_flows=12, n_group=8), "cases": {}}
    for case in args.cases.split(","):
        if case == "b1":
            frames, samples = [870], [256 * 870]
        elif case == "b16":
            frames = [int(n) for n in synth_lengths(16, 1234)[1]]
            samples = [256 * n for n in frames]
        else:
            frames, samples = [63] * 12, [16000] * 12
        B, N, T = len(frames), max(frames), max(samples)
        g = torch.Generator().manual_seed(1)
        mel = (torch.randn(B, 80, N, generator=g) * 0.5 - 4.0).to(dev)
        audio = (0.3 * torch.randn(B, T, generator=g)).to(dev)
        zs = [torch.randn(s, generator=g).to(dev) for s in wg.noise_shapes(B, N)]
        ragged = len(set(samples)) > 1
        r = {"B": B, "samples": sum(samples), "frames": sum(frames)}
        outs = {}
        for prec in args.precisions.split(","):
            wg.precision = prec
            fwd = _ms(lambda: outs.__setitem__(prec, wg((mel, audio), lengths=samples if ragged else None)[0]), args.reps)
            inf = _ms(lambda: wg.infer(mel, 1.0, lengths=frames if ragged else None, z=zs), args.reps)
            nll = _ms(lambda: wg.nll(mel, audio, lengths=samples if ragged else None), args.reps)
            r[prec] = {"forward_ms": round(fwd, 3), "infer_ms": round(inf, 3), "forward_over_infer": round(fwd / inf, 3),
                       "nll_ms": round(nll, 3)}
        for prec in outs:
            if prec != 'fp32' and 'fp32' in outs:
                a, b = outs[prec].double(), outs['fp32'].double()
                r[prec]["z_rel_l2_vs_fp32"] = float((a - b).norm() / b.norm())
        if not args.no_baseline:
            with torch.no_grad():
                ms = _ms(lambda: fr.forward(ref, mel, audio), args.reps)
                r["torch_fp32"] = {"forward_ms": round(ms, 3)}
                if 'fp32' in outs and not ragged:
                    want = fr.forward(ref, mel, audio)[0].double()
                    r["fp32"]["z_rel_l2_vs_torch_fp32"] = float((outs['fp32'].double() - want).norm() / want.norm())
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
