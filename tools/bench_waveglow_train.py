"""Time a WaveGlow training step on the MI355X: ``forward`` alone, ``training_loss`` + ``backward``, their ratio, the float32
restatement's forward + backward under torch autograd on the same GPU (tests/waveglow_fwd_ref.py: the way to train it
without this engine), the bytes kept between forward and backward and the cost of the per-step repack of the weights.
One JSON line per case.

    python tools/bench_waveglow_train.py [--steps 3] [--warmup 1] [--out profiles/waveglow_train_bench.json]
    python tools/bench_waveglow_train.py --one-step fp32      # a single fp32 step of the training shape (for a kernel trace)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import waveglow_fwd_ref as fr  # noqa: E402
import waveglow_ref as wr  # noqa: E402
from tacotron2_amd.waveglow import WaveGlow  # noqa: E402

CASES = [dict(name="training shape", B=12, N=63, T=16000), dict(name="one utterance", B=1, N=870, T=256 * 870)]


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-step", default=None, metavar="PRECISION")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch restatement")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ref = wr.make_ref(C=256, L=8, seed=0, weight_norm=False)
    wg = WaveGlow.from_module(ref).to(dev).train()
    ref = ref.float().to(dev)
    g = torch.Generator().manual_seed(0)
    lines = []
    for case in CASES:
        mel = (torch.randn(case["B"], 80, case["N"], generator=g) * 0.5 - 4.0).to(dev)
        audio = (0.3 * torch.randn(case["B"], case["T"], generator=g)).to(dev)

        def step():
            wg.zero_grad(set_to_none=False)
            wg.training_loss(mel, audio).backward()

        if a.one_step:
            wg.precision = a.one_step
            step()
            step()
            torch.cuda.synchronize()
            return
        rows = case["T"] // 8
        P = wg.forward_plan([rows] * case["B"], [-(-case["T"] // 256)] * case["B"])[3]
        out = dict(case=case["name"], B=case["B"], T=case["T"], N=case["N"], packed_rows=P,
                   saved_state_bytes=wg.saved_state_bytes(P, case["B"] * -(-case["T"] // 256)))

        def repack():
            wg._pack = None
            wg._packed(dev)

        out["repack_ms"] = _median_ms(repack, a.steps, a.warmup)
        for prec in ("fp32", "bf16x3", "bf16"):
            wg.precision = prec
            fwd = _median_ms(lambda: wg((mel, audio)), a.steps, a.warmup)
            trn = _median_ms(step, a.steps, a.warmup)
            out[prec] = dict(forward_ms=fwd, step_ms=trn, ratio=trn / fwd)
        if not a.no_torch:
            def torch_step():
                ref.zero_grad(set_to_none=False)
                fr.loss(fr.forward(ref, mel, audio)).backward()

            out["torch_f32_step_ms"] = _median_ms(torch_step, a.steps, a.warmup)
            for prec in ("fp32", "bf16x3", "bf16"):
                out[prec]["speedup_over_torch"] = out["torch_f32_step_ms"] / out[prec]["step_ms"]
        print(json.dumps(out), flush=True)
        lines.append(out)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
