"""WaveGlow inference on the MI355X: one JSON line.

    python tools/bench_waveglow.py [--reps 3] [--cases b1,b16] [--precisions fp32,bf16x3,bf16] [--no-baseline] [--out F]

Model: the published geometry (80 mels, 12 flows, n_group 8, early outputs of 2 every 4 flows, WN 8 layers of 256
channels) with tests/waveglow_ref.py's seeded weights.  Cases: B = 1 at 870 frames (10.1 s of audio) and B = 16 ragged
(synth_lengths(16, 1234)).  For each case and precision: ms per call (median of `reps` after one warm-up), the real-time
factor (seconds of audio per second), TF/s against the flop count 2 * (3C * 2C * L + 640 * 2CL + res/skip) per row per
flow, the share of its bound (157.3 TF exact f32; bf16x3 three and bf16 one product at 2.5 PF) and the relative L2 of the
waveform against the fp32 mode.  Baseline: the float64-structured restatement (eager conv1d / conv_transpose1d, weight
norm included) run in float32 and in float16 on the same GPU, as the reference notebook runs it.
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

import waveglow_ref as wr  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402
from tacotron2_amd.waveglow import WaveGlow  # noqa: E402

PEAK = {'fp32': 157.3e12, 'bf16x3': 2.5e15 / 3, 'bf16': 2.5e15}
SR = 22050


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


def flops_per_row_flow(C, L, n_mel=80, G=8):
    return 2 * (3 * C * 2 * C * L + n_mel * G * 2 * C * L + (L - 1) * C * 2 * C + C * C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="b1,b16")
    ap.add_argument("--precisions", default="fp32,bf16x3,bf16")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    C, L = 256, 8
    ref = wr.make_ref(C=C, L=L, seed=0)
    wg = WaveGlow.from_module(ref).to(dev).eval()
    ref = ref.to(dev)
    res = {"model": dict(C=C, L=L, n_flows=12, n_group=8), "cases": {}}
    for case in args.cases.split(","):
        if case == "b1":
            lens = [870]
        else:
            lens = [int(n) for n in synth_lengths(16, 1234)[1]]
        B, N = len(lens), max(lens)
        g = torch.Generator().manual_seed(1)
        mel = (torch.randn(B, 80, N, generator=g) * 0.5 - 4.0).to(dev)
        z = [torch.randn(s, generator=g).to(dev) for s in wg.noise_shapes(B, N)]
        rows = 32 * sum(lens)
        flops = flops_per_row_flow(C, L) * 12 * rows
        secs = 256 * sum(lens) / SR
        r = {"B": B, "frames": sum(lens), "audio_s": secs, "gflop": flops / 1e9}
        outs = {}
        for prec in args.precisions.split(","):
            wg.precision = prec
            lj = lens if B > 1 else None
            ms = _ms(lambda: outs.__setitem__(prec, wg.infer(mel, 0.666, lengths=lj, z=z)), args.reps)
            tf = flops / (ms * 1e-3) / 1e12
            r[prec] = {"ms": round(ms, 3), "rtf": round(secs / (ms * 1e-3), 1), "tflops": round(tf, 1),
                       "bound_share": round(tf * 1e12 / PEAK[prec], 3)}
        for prec in outs:
            if prec != 'fp32' and 'fp32' in outs:
                a, b = outs[prec].double(), outs['fp32'].double()
                r[prec]["rel_l2_vs_fp32"] = float((a - b).norm() / b.norm())
        if not args.no_baseline:
            with torch.no_grad():
                for name, dt in (("torch_fp32", torch.float32), ("torch_fp16", torch.float16)):
                    m = ref.to(dt)
                    zz = [t.to(dt) for t in z]
                    ms = _ms(lambda: m.infer(mel.to(dt), 0.666, zz), args.reps)
                    r[name] = {"ms": round(ms, 3), "rtf": round(secs / (ms * 1e-3), 1)}
                ref.float()
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
