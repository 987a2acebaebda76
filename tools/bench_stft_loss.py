"""MultiResolutionSTFTLoss on the MI355X, alone and inside a Vocos fine-tuning step, beside torch autograd: one JSON line.

    python tools/bench_stft_loss.py [--reps 5] [--cases b1,b16] [--precisions fp32,bf16x3] [--no-baseline] [--out F]

Writes the line to profiles/stft_loss_bench.json as well (``--out`` names another file).

Cases are tools/bench_mel_loss.py's: B = 1 at 870 frames and B = 16 ragged (synth_lengths(16, 1234)), the audio 256 x frames
samples of clamp(0.1 randn), the target 0.7 audio + 0.7 clamp(0.1 randn), the default resolutions.  For each case and precision
(of the loss's backward): ms of the forward alone and of forward + backward (median of `reps` after one warm-up, a host clock
around work that ends in a device synchronise), the elements kept between them, and ms per kernel kind of one forward + backward
(every launch between a pair of events, summed by kernel: the sum exceeds the call's time by the event overhead).  The hop-50
resolution (512, 50, 240) alone beside the same resolution at hop 48: its forward GEMM reads the A operand at a row stride that is
no multiple of 4 and its fold takes the scalar path; the per-kernel times of the two say what that costs.  A whole fine-tuning
step (``vocos_train.train_step`` on the published Vocos geometry with seeded weights) at stft_loss_weight 0 and 1, and the step at
weight 0 beside the step as it stood before the second loss existed, written out inline, in the same session: three medians of
each, taken in turn.  In the same process: float32 torch autograd over the restatement (tests/stft_loss_ref.py; its basis tables
are built once, in the warm-up call).  ratio_to_torch is torch's time over this one's
(above 1: this is faster).
"""
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

import stft_loss_ref as sr  # noqa: E402
import vocos_ref as vr  # noqa: E402
from bench_mel_loss import STEP_KERNELS, _ms, kernel_times  # noqa: E402
from tacotron2_amd import vocos_train as vt  # noqa: E402
from tacotron2_amd.audio import MelLoss, MultiResolutionSTFTLoss, TacotronSTFT  # noqa: E402
from tacotron2_amd.optim import FusedAdam  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402
from tacotron2_amd.vocos import load_vocos  # noqa: E402

LOSS_KERNELS = ('reflect_pad', 'gemm', 'stft_loss_fwd', 'stft_loss_finish', 'stft_loss_bwd', 'stft_frames_fold', 'stft_loss_sum')
HOP = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="b1,b16")
    ap.add_argument("--precisions", default="fp32,bf16x3")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stft_loss_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sl = MultiResolutionSTFTLoss().to(dev)
    hop50 = MultiResolutionSTFTLoss(((512, 50, 240),)).to(dev)
    hop48 = MultiResolutionSTFTLoss(((512, 48, 240),)).to(dev)
    ml = MelLoss(TacotronSTFT().to(dev))
    voc = load_vocos(vr.make_ref('V', 0).state_dict()).to(dev).train()
    opt = FusedAdam(voc.parameters(), lr=1e-5)
    res = {"resolutions": [list(r) for r in sl.resolutions], "model": "V", "cases": {}}
    for case in args.cases.split(","):
        frames = [870] if case == "b1" else [int(n) for n in synth_lengths(16, 1234)[1]]
        B, N = len(frames), max(frames)
        lens = [HOP * n for n in frames] if B > 1 else None
        g = torch.Generator().manual_seed(3)
        audio = torch.clamp(0.1 * torch.randn(B, HOP * N, generator=g), -1.0, 1.0).to(dev)
        target = (0.7 * audio + 0.7 * torch.clamp(0.1 * torch.randn(B, HOP * N, generator=g), -1.0, 1.0).to(dev))
        audio.requires_grad_(True)
        mel = vr.make_mel(B, N, 1).to(dev)
        r = {"B": B, "frames": sum(frames), "samples": HOP * N, "kept_elements": sl.kept_state_floats(B, HOP * N)}
        for prec in args.precisions.split(","):
            def loss_step(mod=sl):
                audio.grad = None
                mod(audio, target, lengths=lens, precision=prec).backward()

            def inline_step():                                         # the step before the second loss existed
                voc.zero_grad()
                loss = ml(voc.generate(mel[:, :, :N].contiguous()), mel[:, :, :N], precision=prec)
                loss.backward()
                opt.step()

            voc.precision = prec
            fwd = _ms(lambda: sl(audio.detach(), target, lengths=lens, precision=prec), args.reps)
            both = _ms(loss_step, args.reps)
            step0, before = [], []
            for _ in range(3):                                         # interleaved: three medians of each
                step0.append(round(_ms(lambda: vt.train_step(voc, ml, opt, mel, N, N, prec), args.reps), 3))
                before.append(round(_ms(inline_step, args.reps), 3))
            step1 = _ms(lambda: vt.train_step(voc, ml, opt, mel, N, N, prec, sl, 1.0, target), args.reps)
            r[prec] = {"loss_forward_ms": round(fwd, 3), "loss_forward_backward_ms": round(both, 3),
                       "vocos_step_weight0_ms": step0, "vocos_step_before_ms": before, "vocos_step_weight1_ms": round(step1, 3),
                       "loss_kernels": kernel_times(loss_step, LOSS_KERNELS),
                       "hop50_alone_ms": round(_ms(lambda: loss_step(hop50), args.reps), 3),
                       "hop48_alone_ms": round(_ms(lambda: loss_step(hop48), args.reps), 3),
                       "hop50_kernels": kernel_times(lambda: loss_step(hop50), LOSS_KERNELS),
                       "hop48_kernels": kernel_times(lambda: loss_step(hop48), LOSS_KERNELS),
                       "step_weight1_kernels": kernel_times(lambda: vt.train_step(voc, ml, opt, mel, N, N, prec, sl, 1.0, target),
                                                            STEP_KERNELS + LOSS_KERNELS[2:])}
        if not args.no_baseline:
            x = audio.detach()
            tf = _ms(lambda: sr.loss(x, target, sl.resolutions, lens), args.reps)
            tb = _ms(lambda: sr.loss_and_grad(x, target, sl.resolutions, lens), args.reps)
            r["torch_autograd_fp32"] = {"loss_forward_ms": round(tf, 3), "loss_forward_backward_ms": round(tb, 3)}
            for prec in args.precisions.split(","):
                r[prec]["ratio_to_torch_forward"] = round(tf / r[prec]["loss_forward_ms"], 2)
                r[prec]["ratio_to_torch"] = round(tb / r[prec]["loss_forward_backward_ms"], 2)
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
