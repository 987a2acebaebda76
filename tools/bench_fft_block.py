"""First timings of the feed-forward Transformer block's convolutional feed-forward (transformer.PositionwiseConvFF) and of one
transformer.FFTBlock, forward and forward + backward, against the torch formulation on the padded batch (nn.Conv1d with masks,
F.layer_norm, masked softmax attention), with the peak memory of each.  (d_model, d_inner, k) = (384, 1536, 3) at B = 1, T = 870;
B = 16 at a ragged frame rate; B = 64 at a ragged token rate.  Prints one JSON line and, with --out, writes it.

    python tools/bench_fft_block.py --out profiles/fft_block_bench.json
    python tools/bench_fft_block.py --smallest --iters 2
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tacotron2_amd import transformer  # noqa: E402


def lengths_for(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    ln = (torch.rand(B, generator=g) * 0.6 + 0.4) * T
    ln = ln.round().long().clamp(1, T)
    ln[0] = T
    return ln


def torch_conv_ff(ff, x, mask):
    """The padded-batch formulation: masks before each convolution and after the last."""
    ln = ff.layer_norm
    h = F.layer_norm(x, (x.shape[2],), ln.weight, ln.bias, ln.eps) if ff.pre_lnorm else x
    h = F.relu(ff.conv1((h * mask).transpose(1, 2)))
    h = ff.conv2(h * mask.transpose(1, 2)).transpose(1, 2)
    out = h + x if ff.pre_lnorm else F.layer_norm(h + x, (x.shape[2],), ln.weight, ln.bias, ln.eps)
    return out * mask


def torch_block(blk, x, mask):
    a = blk.dec_attn
    B, T, _ = x.shape
    H, D = a.n_head, a.d_head
    h = a.layer_norm(x) if a.pre_lnorm else x
    q, k, v = (c.view(B, T, H, D).transpose(1, 2) for c in a.qkv_net(h).chunk(3, dim=2))
    s = (q @ k.transpose(2, 3)) * a.scale
    s = s.masked_fill(~mask.bool().view(B, 1, 1, T), float("-inf"))
    o = (torch.softmax(s, dim=3) @ v).transpose(1, 2).reshape(B, T, H * D)
    out = x + a.o_net(o)
    out = out if a.pre_lnorm else a.layer_norm(out)
    return torch_conv_ff(blk.pos_ff, out, mask)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, torch.cuda.max_memory_allocated() - base


def bench_case(name, B, T, d, di, k, iters, warmup):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    ln = lengths_for(B, T, B)
    len_dev = ln.to(torch.int32).to(dev)
    mask = (torch.arange(T)[None, :] < ln[:, None]).float()[:, :, None].to(dev)
    x = torch.randn(B, T, d, device=dev).mul_(mask).requires_grad_(True)
    g = torch.randn(B, T, d, device=dev)
    res = dict(case=name, B=B, T=T, frames=int(ln.sum()), d_model=d, d_inner=di, k=k)
    mods = (("", transformer.PositionwiseConvFF(d, di, k).to(dev), torch_conv_ff),
            ("block_", transformer.FFTBlock(2, d, d // 2 if d // 2 <= 128 else 64, di, k).to(dev), torch_block))
    for tag, mod, ref in mods:
        def nat_f():
            with torch.no_grad():
                mod(x, len_dev)

        def ref_f():
            with torch.no_grad():
                ref(mod, x, mask)

        def nat_fb():
            mod(x, len_dev).backward(g)

        def ref_fb():
            ref(mod, x, mask).backward(g)
        for key, fn in (("native_fwd", nat_f), ("torch_fwd", ref_f), ("native_fwd_bwd", nat_fb), ("torch_fwd_bwd", ref_fb)):
            ms, peak = timed(fn, iters, warmup)
            res[tag + key + "_ms"], res[tag + key + "_peak_bytes"] = round(ms, 4), int(peak)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--smallest", action="store_true", help="one small case: the tool's own test")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.smallest:
        cases = [("smallest", 2, 40, 64, 128, 3)]
    else:
        cases = [("b1_t870", 1, 870, 384, 1536, 3), ("b16_frames", 16, 870, 384, 1536, 3), ("b64_tokens", 64, 160, 384, 1536, 3)]
    out = dict(tool="bench_fft_block", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup,
               cases=[bench_case(*c, a.iters, min(a.warmup, a.iters)) for c in cases])
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
