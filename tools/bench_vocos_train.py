"""Forward + backward of Vocos.generate on the MI355X beside ``infer`` and torch autograd: one JSON line.

    python tools/bench_vocos_train.py [--reps 5] [--cases b1,b16] [--precisions fp32,bf16x3,bf16] [--no-baseline] [--out F]

Writes the line to profiles/vocos_train_bench.json as well (``--out`` names another file).

Model and cases are tools/bench_vocos.py's: the published mel geometry with tests/vocos_ref.py's seeded weights, B = 1 at
870 frames and B = 16 ragged (synth_lengths(16, 1234)).  For each case and precision: ms of ``generate`` + ``backward`` with
the linear loss sum(audio * r) (every parameter and the mels require grad; median of `reps` after one warm-up, a host clock
around work that ends in a device synchronise), ms of ``infer`` at the same shape, ms of the forward of ``generate`` alone,
the bytes kept between forward and backward, and ms per kernel of one forward + backward (every launch between a pair of
events, summed by kernel: the sum exceeds the call's time by the event overhead).  In the same process: float32 torch
autograd over the restatement (tests/vocos_grad_ref.py; the padded batch, as torch runs it).  ratio_to_infer is the step's
time over infer's; ratio_to_torch is torch's time over the step's (above 1: this backward is faster).
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

import vocos_grad_ref as gr  # noqa: E402
import vocos_ref as vr  # noqa: E402
from tacotron2_amd import native as nv  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402
from tacotron2_amd.vocos import load_vocos  # noqa: E402

KERNELS = ('hg_pack_mel', 'hg_conv', 'vc_dwln', 'vc_linear', 'vc_polar', 'vc_ola', 'vc_ola_bwd', 'vc_polar_bwd', 'vc_gelu_bwd',
           'vc_gamma_bwd', 'vc_ln_bwd', 'vc_dw_bwd', 'gemm', 'splitk_reduce2d', 'colsum', 'wg_partial_sum')


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


def kernel_times(step):
    """ms per kernel of one forward + backward: every launch between two events."""
    spans, saved = [], {k: getattr(nv, k) for k in KERNELS}

    def wrap(name, fn):
        def run(*a, **k):
            tag = name
            if name == 'vc_linear':
                tag += ':K%d:N%d' % (a[1].shape[1], a[1].shape[0])
            if name == 'gemm':
                tag += ':wgrad:%dx%d' % tuple(a[0].shape)
            if name in ('vc_dwln', 'vc_ln_bwd'):
                tag += ':ln' if a[1] is None else ':dwconv'
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(*a, **k)
            e1.record()
            spans.append((tag, e0, e1))
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
    ap.add_argument("--precisions", default="fp32,bf16x3,bf16")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocos_train_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ref = vr.make_ref('V', 0)
    voc = load_vocos(ref.state_dict()).to(dev)
    res = {"model": "V", "saved_bytes_per_frame": voc.saved_state_bytes(1), "cases": {}}
    for case in args.cases.split(","):
        lens = [870] if case == "b1" else [int(n) for n in synth_lengths(16, 1234)[1]]
        B, N = len(lens), max(lens)
        mel = vr.make_mel(B, N, 1).to(dev).requires_grad_(True)
        lj = lens if B > 1 else None
        w = gr.loss_weights((B, 1, voc.samples(N)), 2).float().to(dev)
        P = voc.packed_plan(lens)[4]
        r = {"B": B, "frames": sum(lens), "packed_rows": P, "saved_state_gb": round(voc.saved_state_bytes(P) / 1e9, 3)}

        def step():
            voc.generate(mel, lengths=lj).backward(w)

        for prec in args.precisions.split(","):
            voc.precision = prec
            ms = _ms(step, args.reps)
            fwd = _ms(lambda: voc.generate(mel, lengths=lj), args.reps)
            inf = _ms(lambda: voc.infer(mel.detach(), lengths=lj), args.reps)
            r[prec] = {"ms": round(ms, 3), "generate_forward_ms": round(fwd, 3), "infer_ms": round(inf, 3),
                       "ratio_to_infer": round(ms / inf, 2), "kernels": kernel_times(step)}
        if not args.no_baseline:
            ref32 = ref.to(dev).float()
            x = mel.detach()
            ms = _ms(lambda: gr.grads(ref32, x, w), args.reps)
            r["torch_autograd_fp32"] = {"ms": round(ms, 3), "frames_computed": B * N}
            for prec in args.precisions.split(","):
                r[prec]["ratio_to_torch"] = round(ms / r[prec]["ms"], 2)
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
