"""Griffin-Lim on the MI355X: one JSON line.

    python tools/bench_griffin_lim.py [--iters 60] [--reps 3] [--cases b1,b64] [--precisions fp32,bf16x3] [--no-baseline]

Cases: B = 1 at 870 frames and B = 64 ragged (synth_lengths(64, 1234), the flagship batch's mel lengths).  For each case
and precision: ms per call (griffin_lim with `iters` iterations, initial angles given, median of `reps` calls after one
warm-up), ms per iteration, seconds of audio per second, the packed row count, GEMM flops and element-pass bytes computed
from the shapes, and the shares of the MFMA peak (157.3 TF exact f32; 2.5 PF bf16, of which split-bf16 uses 3 products)
and of HBM (8 TB/s), MI355X_MICROARCH.md.  Baseline: the reference's arithmetic (stft.py transform / inverse,
audio_processing.griffin_lim: conv1d / conv_transpose1d over the zero-padded batch, window_sumsquare in numpy and copied
to the device on every inverse) restated with torch on the same GPU.  MIOPEN_FIND_MODE defaults to FAST here: the
exhaustive per-shape algorithm search of the default mode takes minutes at these convolution shapes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

# the baseline's convolutions: MIOpen's heuristic algorithm choice, not the exhaustive per-shape search (minutes here)
os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tacotron2_amd import audio  # noqa: E402
from tacotron2_amd.synth import synth_lengths  # noqa: E402

PEAK_F32 = 157.3e12
PEAK_BF16 = 2.5e15
HBM = 8.0e12
SR = 22050


def _sync_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


class RefTorch:
    """reference stft.py:42-141 + audio_processing.py:59-76, float32, torch on the device (the padded batch)."""

    def __init__(self, stft, dev):
        L, F = stft.filter_length, stft.cutoff
        self.L, self.hop, self.win, self.F = L, stft.hop_length, stft.win_length, F
        fb = audio.fourier_basis(L, stft.win_length)                 # windowed, == the reference's forward_basis
        self.fwd = torch.from_numpy(fb)[:, None, :].to(dev)
        self.inv = torch.from_numpy(audio.inverse_basis(L, self.hop, self.win).copy())[:, None, :].to(dev)

    def transform(self, x):
        B, T = x.shape
        xp = Fn.pad(x.view(B, 1, 1, T), (self.L // 2, self.L // 2, 0, 0), mode='reflect').squeeze(1)
        ft = Fn.conv1d(xp, self.fwd, stride=self.hop)
        re, im = ft[:, :self.F], ft[:, self.F:]
        return torch.sqrt(re ** 2 + im ** 2), torch.atan2(im, re)

    def inverse(self, mag, phase):
        rec = torch.cat([mag * torch.cos(phase), mag * torch.sin(phase)], dim=1)
        out = Fn.conv_transpose1d(rec, self.inv, stride=self.hop)
        ws = audio.window_sumsquare('hann', mag.size(-1), hop_length=self.hop, win_length=self.win, n_fft=self.L)
        idx = torch.from_numpy(np.where(ws > np.finfo(np.float32).tiny)[0]).to(mag.device)
        ws = torch.from_numpy(ws).to(mag.device)
        out[:, :, idx] /= ws[idx]
        out *= float(self.L) / self.hop
        return out[:, :, self.L // 2:-(self.L // 2)]

    def griffin_lim(self, mag, angles, n_iters):
        x = self.inverse(mag, angles).squeeze(1)
        for _ in range(n_iters):
            _, ph = self.transform(x)
            x = self.inverse(mag, ph).squeeze(1)
        return x


def case_line(name, lengths, precision, iters, reps, stft, baseline):
    dev = torch.device("cuda", 0)
    L, hop, F = stft.filter_length, stft.hop_length, stft.cutoff
    Fp = (F + 15) // 16 * 16
    B, n = len(lengths), max(lengths)
    gen = torch.Generator().manual_seed(0)
    mag = torch.zeros(B, F, n)
    for b, nb in enumerate(lengths):
        mag[b, :, :nb] = torch.rand(F, nb, generator=gen)
    mag = mag.to(dev)
    np.random.seed(0)
    ang = torch.from_numpy(np.angle(np.exp(2j * np.pi * np.random.rand(B, F, n))).astype(np.float32)).to(dev)
    lens = None if B == 1 else lengths
    ms = _sync_ms(lambda: audio.griffin_lim(mag, stft, n_iters=iters, angles=ang, lengths=lens, precision=precision), reps)
    ms0 = _sync_ms(lambda: audio.griffin_lim(mag, stft, n_iters=0, angles=ang, lengths=lens, precision=precision), reps)
    R = audio.packed_rows(lengths, L, hop)
    flop_it = 2.0 * R * L * (2 * Fp) + 2.0 * R * (2 * F) * L             # inverse + forward GEMM
    P = R * hop + L
    # bytes of one iteration through HBM: GEMM operands/results once each, element passes read + write
    bytes_it = 4.0 * (R * 2 * Fp + R * L) + 4.0 * (R * L + P) + 4.0 * (P + R * 2 * F) + 4.0 * (R * 2 * F + R * F + R * 2 * Fp)
    it_ms = (ms - ms0) / iters
    audio_s = sum((nb - 1) * hop for nb in lengths) / SR
    peak = PEAK_F32 if precision == 'fp32' else PEAK_BF16 / 3.0
    line = {"case": name, "precision": precision, "B": B, "frames": int(sum(lengths)), "packed_rows": R,
            "padded_rows": B * n, "iters": iters, "ms_per_call": round(ms, 3), "ms_per_iter": round(it_ms, 4),
            "audio_s_per_s": round(audio_s / (ms / 1e3), 1), "gemm_gflop_per_iter": round(flop_it / 1e9, 2),
            "hbm_gb_per_iter": round(bytes_it / 1e9, 3),
            "mfma_peak_share": round(flop_it / (it_ms / 1e3) / peak, 3),
            "hbm_share_at_peak_bytes": round(bytes_it / (it_ms / 1e3) / HBM, 3)}
    print("  %s %s: native %.2f ms per call" % (name, precision, ms), file=sys.stderr, flush=True)
    if baseline:
        try:
            ref = RefTorch(stft, dev)
            magp = mag.clone()
            b0 = _sync_ms(lambda: ref.griffin_lim(magp, ang, 0), 1)
            print("  %s torch reference, 0 iterations: %.1f ms" % (name, b0), file=sys.stderr, flush=True)
            bms = _sync_ms(lambda: ref.griffin_lim(magp, ang, iters), max(1, reps - 1))
            print("  %s torch reference, %d iterations: %.1f ms" % (name, iters, bms), file=sys.stderr, flush=True)
            line["torch_ref_ms_per_call"] = round(bms, 3)
            line["torch_ref_ms_per_iter"] = round((bms - b0) / iters, 3)
            line["speedup_vs_torch_ref"] = round(bms / ms, 2)
        except Exception as e:          # e.g. no GPU convolution in this torch build
            line["torch_ref_ms_per_call"] = None
            line["torch_ref_error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="b1,b64")
    ap.add_argument("--precisions", default="fp32,bf16x3")
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    from tacotron2_amd import native
    native.load()
    stft = audio.TacotronSTFT().stft_fn
    cases = {"b1": [870], "b64": [int(v) for v in synth_lengths(64, 1234)[1]]}
    t0 = time.time()
    out = {"tool": "bench_griffin_lim", "library_sha1": native.library_sha1(),
           "device": torch.cuda.get_device_name(0), "results": []}
    for c in args.cases.split(","):
        for p in args.precisions.split(","):
            out["results"].append(case_line(c, cases[c], p, args.iters, args.reps, stft, not args.no_baseline))
            print("[%.0f s] %s" % (time.time() - t0, json.dumps(out["results"][-1])), file=sys.stderr, flush=True)
    out["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
