"""audio.Resample on the MI355X beside the float32 torch ``conv1d`` formulation of its restatement: one JSON line.

    python tools/bench_resample.py [--reps 5] [--inner 20] [--pairs 48000:22050,24000:22050,22050:16000] [--out F]

Writes the line to profiles/resample_bench.json as well (``--out`` names another file).

Cases: for every rate pair, B = 1 x 10 s of clamp(0.1 randn) and B = 16 ragged (synth_lengths(16, 1234) frames of 256 samples at
22 050 Hz, scaled to the source rate).  For each: ms per call of the forward alone and of forward + backward (a host clock around
`inner` calls that end in one device synchronise, divided by `inner`; median of `reps` after a warm-up), the same for the float32
torch formulation in the same process (tests/resample_ref.py: dense table, zero padding, ``conv1d`` at stride o, its autograd; the
table is built once, outside the timed calls), and ms per launch of the two kernels (each launch between a pair of events, mean
of `inner`).  achieved_GBps is the algorithmic traffic of the forward, 4 (T + T') bytes per utterance summed over the batch, over
the forward kernel's event time; the backward moves the same bytes.  ratio_to_torch is torch's time over this one's (above 1: this
is faster)."""
import argparse
import json
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import resample_ref as rr  # noqa: E402
from bench_mel_loss import _ms, kernel_times  # noqa: E402
from tacotron2_amd.audio import Resample  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--pairs", default="48000:22050,24000:22050,22050:16000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"inner": args.inner, "reps": args.reps, "cases": {}}
    for pair in args.pairs.split(","):
        orig, new = (int(v) for v in pair.split(":"))
        mod = Resample(orig, new).to(dev)
        table = rr.dense_table(orig, new, dtype=torch.float32).to(dev)
        for case in ("b1", "b16"):
            lens = [10 * orig] if case == "b1" else [int(256 * n * orig / 22050) for n in synth_lengths(16, 1234)[1]]
            B, T = len(lens), max(lens)
            ragged = lens if B > 1 else None
            g = torch.Generator().manual_seed(3)
            x = torch.clamp(0.1 * torch.randn(B, T, generator=g), -1.0, 1.0).to(dev).requires_grad_(True)
            gy = torch.clamp(0.1 * torch.randn(B, mod.output_length(T), generator=g), -1.0, 1.0).to(dev)

            def ours(backward):
                for _ in range(args.inner):
                    out = mod(x if backward else x.detach(), ragged)
                    if backward:
                        x.grad = None
                        (out if ragged is None else out[0]).backward(gy)

            def theirs(backward):
                for _ in range(args.inner):
                    out = rr.resample(x if backward else x.detach(), orig, new, lengths=ragged, table=table)
                    if backward:
                        x.grad = None
                        out.backward(gy)

            t = {"ours_fwd": _ms(lambda: ours(False), args.reps) / args.inner, "ours_both": _ms(lambda: ours(True), args.reps) / args.inner,
                 "torch_fwd": _ms(lambda: theirs(False), args.reps) / args.inner,
                 "torch_both": _ms(lambda: theirs(True), args.reps) / args.inner}
            kt = kernel_times(lambda: ours(True), ("resample_fwd", "resample_bwd"))
            k_fwd = kt["resample_fwd"]["ms"] / kt["resample_fwd"]["launches"]
            k_bwd = kt["resample_bwd"]["ms"] / kt["resample_bwd"]["launches"]
            nbytes = 4 * sum(n + mod.output_length(n) for n in lens)
            r = {"B": B, "samples": T, "sum_samples": sum(lens), "table_paths": list(mod.table_paths()),
                 "forward_ms": round(t["ours_fwd"], 4), "forward_backward_ms": round(t["ours_both"], 4),
                 "torch_conv1d_fp32": {"forward_ms": round(t["torch_fwd"], 4), "forward_backward_ms": round(t["torch_both"], 4)},
                 "ratio_to_torch_forward": round(t["torch_fwd"] / t["ours_fwd"], 2),
                 "ratio_to_torch": round(t["torch_both"] / t["ours_both"], 2),
                 "kernel_ms": {"resample_fwd": round(k_fwd, 4), "resample_bwd": round(k_bwd, 4)},
                 "algorithmic_bytes": nbytes,
                 "achieved_GBps": {"resample_fwd": round(nbytes / k_fwd / 1e6, 1), "resample_bwd": round(nbytes / k_bwd / 1e6, 1)}}
            res["cases"]["%d_%d_%s" % (orig, new, case)] = r
            print(pair, case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
