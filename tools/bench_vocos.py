"""Vocos on the MI355X beside the HiFi-GAN V1 generator: one JSON line.

    python tools/bench_vocos.py [--reps 5] [--cases b1,b16] [--precisions fp32,bf16x3,bf16] [--no-baseline] [--out F]

Writes the line to profiles/vocos_bench.json as well (``--out`` names another file).

Model: the published mel geometry (80 mels, dim 512, intermediate 1536, 8 blocks, n_fft 1024, hop 256) with
tests/vocos_ref.py's seeded weights.  Cases: B = 1 at 870 frames (10.1 s of audio) and B = 16 ragged (synth_lengths(16, 1234)),
the cases of tools/bench_hifigan.py.  For each case and precision: ms per call (median of `reps` after one warm-up, a host
clock around work that ends in a device synchronise), the real-time factor, TF/s and TB/s against the flop and byte counts
of the loaded shapes (2 x rows x N x K per product over the real rows; every launch reads its operands once and writes its
result once, f32, no fusion between launches), the relative L2 against the fp32 mode, and ms per kernel (every launch of one
call between a pair of events, summed by kernel: the sum exceeds the call's time by the event overhead).  In the same
process: ``hifigan.Generator.infer`` at V1 in the same precision, and the torch restatement of Vocos in float32 and with a
float16 backbone and head (padded batch, as torch runs it; its inverse STFT stays float32).  ratio_to_hifigan and
ratio_to_torch_fp32 are times over Vocos' time (above 1: Vocos is faster).
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

import hifigan_ref as hr  # noqa: E402
import vocos_ref as vr  # noqa: E402
from tacotron2_amd import native as nv  # noqa: E402
from tacotron2_amd.hifigan import load_hifigan  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402
from tacotron2_amd.vocos import load_vocos  # noqa: E402

SR = 22050
KERNELS = ('hg_pack_mel', 'hg_conv', 'vc_dwln', 'vc_linear', 'vc_polar', 'vc_ola')


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


def per_frame(voc):
    """{part: (flops, f32 bytes moved)} per mel frame from the module's shapes, no fusion between launches."""
    nm, D, I, L = voc.n_mel_channels, voc.dim, voc.intermediate_dim, voc.n_fft
    two_f, nb = L + 2, voc.num_layers
    return collections.OrderedDict([
        ("embed", (2 * D * 7 * nm, 4 * (nm + D))),
        ("norms", (2 * 8 * D, 4 * 2 * 2 * D)),                                    # the LayerNorm after embed and the final one
        ("dwconv_ln", (nb * (2 * 7 * D + 8 * D), nb * 4 * 2 * D)),
        ("pwconv1", (nb * 2 * D * I, nb * 4 * (D + I))),
        ("pwconv2", (nb * 2 * I * D, nb * 4 * (I + 2 * D))),                       # reads the intermediate and the residual
        ("head", (2 * D * two_f, 4 * (D + two_f))),
        ("polar", (0, 4 * 2 * two_f)),
        ("inverse_dft", (2 * two_f * L, 4 * (two_f + L))),
        ("overlap_add", (2 * L, 4 * (L + voc.hop))),
    ])


def kernel_times(voc, mel, lens):
    """ms per kernel of one call: every launch between two events."""
    spans, saved = [], {k: getattr(nv, k) for k in KERNELS}

    def wrap(name, fn):
        def run(*a, **k):
            tag = name
            if name == 'vc_linear':
                tag += {None: ':bias', 'gelu': ':gelu', 'residual': ':residual'}[a[3]] + (':N%d' % a[1].shape[0])
            if name == 'vc_dwln':
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
        voc.infer(mel, lengths=lens)
        torch.cuda.synchronize()
    finally:
        for k, fn in saved.items():
            setattr(nv, k, fn)
    out = collections.OrderedDict()
    for tag, e0, e1 in spans:
        ms, n = out.get(tag, (0.0, 0))
        out[tag] = (ms + e0.elapsed_time(e1), n + 1)
    return {tag: {"ms": round(ms, 4), "launches": n} for tag, (ms, n) in out.items()}


def torch_half(ref16, ref32):
    def run(x16):
        with torch.no_grad():
            m, p = ref16.head(ref16.backbone(x16))
            m, p = m.float(), p.float()
            mag = torch.clamp(torch.exp(m), max=vr.CLAMP)
            c = ref32.config
            return vr.istft(torch.complex(mag * torch.cos(p), mag * torch.sin(p)), ref32.w['head.istft.window'], c['hop_length'],
                            c['padding'])
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="b1,b16")
    ap.add_argument("--precisions", default="fp32,bf16x3,bf16")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocos_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ref = vr.make_ref('V', 0)
    voc = load_vocos(ref.state_dict()).to(dev).eval()
    parts = per_frame(voc)
    flops_f, bytes_f = sum(f for f, _ in parts.values()), sum(b for _, b in parts.values())
    res = {"model": "V", "mflop_per_frame": round(flops_f / 1e6, 2), "kbyte_per_frame": round(bytes_f / 1e3, 1),
           "mflop_per_frame_by_part": {k: round(f / 1e6, 3) for k, (f, _) in parts.items()},
           "kbyte_per_frame_by_part": {k: round(b / 1e3, 2) for k, (_, b) in parts.items()}, "cases": {}}
    hg = None
    if not args.no_baseline:
        hg = load_hifigan({'generator': hr.make_ref('V1', 0).state_dict(weight_norm=True)}).to(dev).eval()
        ref32, ref16 = ref.to(dev).float(), ref.to(dev).half()
        half = torch_half(ref16, ref32)
    for case in args.cases.split(","):
        lens = [870] if case == "b1" else [int(n) for n in synth_lengths(16, 1234)[1]]
        B, N = len(lens), max(lens)
        mel = vr.make_mel(B, N, 1).to(dev)
        lj = lens if B > 1 else None
        secs = 256 * sum(lens) / SR
        flops, byts = flops_f * sum(lens), bytes_f * sum(lens)
        r = {"B": B, "frames": sum(lens), "audio_s": round(secs, 2), "gflop": round(flops / 1e9, 2), "gbyte": round(byts / 1e9, 3)}
        outs = {}
        for prec in args.precisions.split(","):
            voc.precision = prec
            ms = _ms(lambda: outs.__setitem__(prec, voc.infer(mel, lengths=lj)), args.reps)
            r[prec] = {"ms": round(ms, 3), "rtf": round(secs / (ms * 1e-3), 1), "tflops": round(flops / (ms * 1e-3) / 1e12, 3),
                       "tbytes_per_s": round(byts / (ms * 1e-3) / 1e12, 3), "kernels": kernel_times(voc, mel, lj)}
            if hg is not None:
                hg.precision = prec
                hms = _ms(lambda: hg.infer(mel, lengths=lj), args.reps)
                r[prec]["hifigan_ms"] = round(hms, 3)
                r[prec]["ratio_to_hifigan"] = round(hms / ms, 2)
        for prec in outs:
            if prec != 'fp32' and 'fp32' in outs:
                a, b = outs[prec].double(), outs['fp32'].double()
                r[prec]["rel_l2_vs_fp32"] = float((a - b).norm() / b.norm())
        if not args.no_baseline:
            x32, x16 = mel, mel.half()
            for name, fn in (("torch_fp32", lambda: ref32(x32)), ("torch_fp16", lambda: half(x16))):
                ms = _ms(fn, args.reps)
                r[name] = {"ms": round(ms, 3), "rtf": round(secs / (ms * 1e-3), 1), "frames_computed": B * N}
            if 'fp32' in r:
                r['fp32']["ratio_to_torch_fp32"] = round(r["torch_fp32"]["ms"] / r['fp32']["ms"], 2)
        res["cases"][case] = r
        print(case, json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
