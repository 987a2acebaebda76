"""Price training under weight norm on the MI355X at the training shape (B = 12, T = 16000, published geometry), in one
process: the folded step and the weight-normed step (``training_loss`` + ``backward`` with the weights repacked every step,
as after an optimiser step), the two launches of csrc/waveglow_wn.hip alone (events around 100 repeats, bytes moved and the
fraction of the HBM rate achieved) and torch autograd through the float32 weight-normed restatement
(tests/waveglow_ref.make_ref(weight_norm=True)).  The weight-normed step minus the folded step of the same run is the cost of
the feature.  One JSON object.

    python tools/bench_waveglow_wn.py [--steps 3] [--warmup 1] [--out profiles/waveglow_wn_bench.json]
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
from tacotron2_amd import native as nv  # noqa: E402
from tacotron2_amd.waveglow import WaveGlow, fold_weight_norm  # noqa: E402

HBM_GBS = 6290.0            # the HBM rate a float4 copy reaches on the MI355X (8000 GB/s on paper): what the fractions are against


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


def _event_ms(fn, repeats):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(repeats):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ref = wr.make_ref(C=256, L=8, seed=0, weight_norm=True)
    normed = WaveGlow.from_module(ref, weight_norm=True).to(dev).train()
    folded = WaveGlow.from_state_dict(fold_weight_norm(normed.state_dict())).to(dev).train()
    ref = ref.float().to(dev)
    g = torch.Generator().manual_seed(0)
    B, N, T = 12, 63, 16000
    mel = (torch.randn(B, 80, N, generator=g) * 0.5 - 4.0).to(dev)
    audio = (0.3 * torch.randn(B, T, generator=g)).to(dev)
    out = dict(B=B, T=T, N=N, library=nv.library_sha1())

    def stepper(m):
        def step():
            m._pack = None                       # what an optimiser step does to the packed weights
            m.zero_grad(set_to_none=False)
            m.training_loss(mel, audio).backward()
        return step

    for prec in ("fp32", "bf16x3", "bf16"):
        folded.precision = normed.precision = prec
        f = _median_ms(stepper(folded), a.steps, a.warmup)
        n = _median_ms(stepper(normed), a.steps, a.warmup)
        out[prec] = dict(folded_step_ms=f, weight_normed_step_ms=n, cost_ms=n - f)

    wn = normed._wn
    elems = sum(int(r) * int(ln) for _, _, _, r, ln, _ in wn['host'].tolist())
    rows = sum(int(r) for _, _, _, r, _, _ in wn['host'].tolist())
    gout = torch.randn(normed._grad_layout()[0], device=dev)
    dvg = torch.empty(wn['v'].numel() + wn['g'].numel(), device=dev)
    dv, dg = dvg[:wn['v'].numel()], dvg[wn['v'].numel():]
    # checked once through the wrappers, then timed on the entry points themselves (the wrappers walk the table on the host)
    nv.wg_weight_norm(wn['table'], wn['host'], wn['n_units'], wn['v'], wn['g'], wn['w'], wn['norm'])
    nv.wg_weight_norm_bwd(wn['table'], wn['host'], wn['n_units'], gout, wn['v'], wn['g'], wn['norm'], dg, dv, 1.0)
    lib, p, nseg, units = nv.load(), nv.ptr, int(wn['host'].shape[0]), int(wn['n_units'])
    tab = p(wn['table'], torch.int64)
    fold_ms = _event_ms(lambda: nv._check(lib.t2amd_wg_weight_norm_f32(tab, nseg, units, p(wn['v']), p(wn['g']), p(wn['w']),
                                                                       p(wn['norm']), nv._stream()), "fold"), a.repeats)
    bwd_ms = _event_ms(lambda: nv._check(lib.t2amd_wg_weight_norm_bwd_f32(tab, nseg, units, p(gout), p(wn['v']), p(wn['g']),
                                                                          p(wn['norm']), p(dg), p(dv), 1.0, nv._stream()),
                                         "backward"), a.repeats)
    fold_b, bwd_b = 4 * (2 * elems + 2 * rows), 4 * (3 * elems + 3 * rows)
    out["launches"] = dict(tensors=int(wn['host'].shape[0]), rows=rows, elements=elems, work_units=int(wn['n_units']),
                           fold_ms=fold_ms, fold_bytes=fold_b, fold_GBs=fold_b / fold_ms / 1e6,
                           fold_fraction_of_hbm=fold_b / fold_ms / 1e6 / HBM_GBS,
                           backward_ms=bwd_ms, backward_bytes=bwd_b, backward_GBs=bwd_b / bwd_ms / 1e6,
                           backward_fraction_of_hbm=bwd_b / bwd_ms / 1e6 / HBM_GBS,
                           note="events around %d back-to-back launches" % a.repeats)

    def torch_step():
        ref.zero_grad(set_to_none=False)
        fr.loss(fr.forward(ref, mel, audio)).backward()

    out["torch_f32_weight_normed_step_ms"] = _median_ms(torch_step, a.steps, a.warmup)
    for prec in ("fp32", "bf16x3", "bf16"):
        out[prec]["speedup_over_torch"] = out["torch_f32_weight_normed_step_ms"] / out[prec]["weight_normed_step_ms"]
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
