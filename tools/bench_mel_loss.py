"""MelLoss on the MI355X, alone and at the end of a Vocos fine-tuning step, beside torch autograd: one JSON line.

    python tools/bench_mel_loss.py [--reps 5] [--cases b1,b16] [--precisions fp32,bf16x3] [--no-baseline] [--out F]

Writes the line to profiles/mel_loss_bench.json as well (``--out`` names another file).

Cases are tools/bench_vocos_train.py's: B = 1 at 870 frames and B = 16 ragged (synth_lengths(16, 1234)), the audio hop x
frames samples of clamp(0.1 randn), the targets seeded log-mel-like values.  For each case and precision (of the loss's
backward): ms of the ``MelLoss`` forward alone, ms of forward + backward (median of `reps` after one warm-up, a host clock
around work that ends in a device synchronise), the floats kept between them, and ms per kernel of one forward + backward
(every launch between a pair of events, summed by kernel: the sum exceeds the call's time by the event overhead).  A whole
fine-tuning step (``generate`` -> ``MelLoss`` -> ``backward`` -> ``FusedAdam``) on the published Vocos geometry with seeded
weights is timed the same way, model and loss at the same precision.  In the same process: float32 torch autograd over the
restatement (tests/audio_grad_ref.py) of the loss alone.  ratio_to_torch is torch's time over this one's (above 1: this is
faster).
"""
import argparse
import collections
import json
import os
import sys
import time

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import audio_grad_ref as ar  # noqa: E402
import vocos_ref as vr  # noqa: E402
from tacotron2_amd import native as nv  # noqa: E402
from tacotron2_amd.audio import MelLoss, TacotronSTFT  # noqa: E402
from tacotron2_amd.optim import FusedAdam  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402
from tacotron2_amd.vocos import load_vocos  # noqa: E402

LOSS_KERNELS = ('reflect_pad', 'stft_magnitude', 'mel_log_compress', 'mel_l1_fwd', 'mel_l1_bwd', 'mel_log_bwd',
                'stft_magnitude_bwd', 'stft_frames_fold', 'gemm', 'wg_partial_sum')
STEP_KERNELS = LOSS_KERNELS + ('hg_pack_mel', 'hg_conv', 'vc_dwln', 'vc_linear', 'vc_polar', 'vc_ola', 'vc_ola_bwd',
                               'vc_polar_bwd', 'vc_gelu_bwd', 'vc_gamma_bwd', 'vc_ln_bwd', 'vc_dw_bwd', 'splitk_reduce2d',
                               'colsum', 'adam_step')


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


def kernel_times(step, kernels):
    """ms per kernel kind of one call of ``step``: every launch between two events."""
    spans, saved = [], {k: getattr(nv, k) for k in kernels if hasattr(nv, k)}

    def wrap(name, fn):
        def run(*a, **k):
            tag = name
            if name == 'gemm':
                tag += ':%dx%d' % (a[0].shape[-1], a[1].shape[-1])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            spans.append((tag, e0, e1))
            return out
        return run

    try:
        for k, fn in saved.items():
            setattr(nv, k, wrap(k, fn))
        step()
        torch.cuda.synchronize()
    finally:
        for k, fn in saved.items():
            setattr(nv, k, fn)
    out = collections.OrderedDict()
    for tag, e0, e1 in spans:
        ms, n = out.get(tag, (0.0, 0))
        out[tag] = (ms + e0.elapsed_time(e1), n + 1)
    return {tag: {"ms": round(ms, 4), "launches": n} for tag, (ms, n) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="b1,b16")
    ap.add_argument("--precisions", default="fp32,bf16x3")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_loss_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    st = TacotronSTFT().to(dev)
    ml = MelLoss(st)
    voc = load_vocos(vr.make_ref('V', 0).state_dict()).to(dev).train()
    opt = FusedAdam(voc.parameters(), lr=1e-5)
    hop = st.stft_fn.hop_length
    res = {"geometry": dict(ar.DEFAULT), "model": "V", "cases": {}}
    for case in args.cases.split(","):
        lens = [870] if case == "b1" else [int(n) for n in synth_lengths(16, 1234)[1]]
        B, N = len(lens), max(lens)
        lj = lens if B > 1 else None
        g = torch.Generator().manual_seed(3)
        audio = torch.clamp(0.1 * torch.randn(B, hop * N, generator=g), -1.0, 1.0).to(dev).requires_grad_(True)
        target = vr.make_mel(B, N, 1).to(dev)
        r = {"B": B, "frames": sum(lens), "samples": hop * N, "kept_floats": st.kept_state_floats(B, hop * N)}
        for prec in args.precisions.split(","):
            def loss_step():
                audio.grad = None
                ml(audio, target, lengths=lj, precision=prec).backward()

            def train_step():
                voc.zero_grad()
                ml(voc.generate(target, lengths=lj), target, lengths=lj, precision=prec).backward()
                opt.step()

            voc.precision = prec
            fwd = _ms(lambda: ml(audio.detach(), target, lengths=lj, precision=prec), args.reps)
            both = _ms(loss_step, args.reps)
            step = _ms(train_step, args.reps)
            r[prec] = {"loss_forward_ms": round(fwd, 3), "loss_forward_backward_ms": round(both, 3),
                       "vocos_step_ms": round(step, 3), "loss_kernels": kernel_times(loss_step, LOSS_KERNELS),
                       "step_kernels": kernel_times(train_step, STEP_KERNELS)}
        if not args.no_baseline:
            x, t64 = audio.detach(), target.double()
            tf = _ms(lambda: ar.l1_loss(ar.logmel(x, ar.DEFAULT), t64, lj), args.reps)
            tb = _ms(lambda: ar.loss_and_grad_l1(x, ar.DEFAULT, t64, lj), args.reps)
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
