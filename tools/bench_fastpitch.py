"""First timings of the thin ends of a temporal predictor (fastpitch.channel_project, fastpitch.scalar_embed), of one
fastpitch.TemporalPredictor, of fastpitch.FastPitch forward + backward under FastPitchLoss and of FastPitch.infer, against the
float32 torch formulation on the padded batch with masks (nn.Linear, nn.Conv1d, F.layer_norm, masked softmax attention,
repeat_interleave), with the peak memory of each.  The model is the default FastPitch (d_model 384, 6 + 6 layers, filter 256) at
B = 1 with 187 tokens, B = 16 ragged, B = 64 at the token rate.  Prints one JSON line and, with --out, writes it.

    python tools/bench_fastpitch.py --out profiles/fastpitch_bench.json
    python tools/bench_fastpitch.py --smallest --iters 2
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tacotron2_amd import fastpitch  # noqa: E402
from tacotron2_amd.transformer import positional_embedding  # noqa: E402
from bench_fft_block import lengths_for, timed, torch_block  # noqa: E402


def torch_predictor(tp, x, mask):
    h = x
    for layer in tp.layers:
        h = F.relu(layer.conv((h * mask).transpose(1, 2))).transpose(1, 2)
        h = F.layer_norm(h, (h.shape[2],), layer.norm.weight, layer.norm.bias, layer.norm.eps)
    y = tp.fc(h) * mask
    return y.squeeze(2) if tp.n_predictions == 1 else y


def torch_transformer(net, x, mask):
    h = (x + positional_embedding(x.shape[1], net.d_model, None, x.device)) * mask
    for layer in net.layers:
        h = torch_block(layer, h, mask)
    return h


def torch_model(model, text, durations, pitch, n_mask, T):
    """The padded-batch formulation of FastPitch.forward: masks around every convolution, repeat_interleave per utterance."""
    enc = torch_transformer(model.encoder, model.encoder.word_emb(text), n_mask)
    log_dur = torch_predictor(model.duration_predictor, enc, n_mask)
    pitch_pred = torch_predictor(model.pitch_predictor, enc, n_mask)
    h = (enc + model.pitch_emb((pitch * n_mask[:, :, 0])[:, None]).transpose(1, 2)) * n_mask
    rows = [torch.repeat_interleave(h[b], durations[b].long(), dim=0)[:T] for b in range(h.shape[0])]
    frames = torch.stack([F.pad(r, (0, 0, 0, T - r.shape[0])) for r in rows])
    t_len = torch.tensor([r.shape[0] for r in rows], device=h.device)
    t_mask = (torch.arange(T, device=h.device)[None, :] < t_len[:, None]).float()[:, :, None]
    dec = torch_transformer(model.decoder, frames, t_mask)
    return model.proj(dec) * t_mask, t_len, log_dur, pitch_pred, None


def bench_case(name, B, N, cfg, iters, warmup):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    ln = lengths_for(B, N, B)
    n_dev = ln.to(torch.int32).to(dev)
    n_mask = (torch.arange(N)[None, :] < ln[:, None]).float()[:, :, None].to(dev)
    d = cfg.get("d_model", 384)
    res = dict(case=name, B=B, N=N, tokens=int(ln.sum()), d_model=d)

    def record(key, fn):
        ms, peak = timed(fn, iters, warmup)
        res[key + "_ms"], res[key + "_peak_bytes"] = round(ms, 4), int(peak)

    # the two thin ops, forward and forward + backward
    h = torch.randn(B, N, d, device=dev).mul_(n_mask).requires_grad_(True)
    v = torch.randn(B, N, device=dev).mul_(n_mask[:, :, 0])
    lin, conv = torch.nn.Linear(d, 1).to(dev), torch.nn.Conv1d(1, d, 3, padding=1).to(dev)
    g1, gd = torch.randn(B, N, 1, device=dev), torch.randn(B, N, d, device=dev)
    ops = (("project", lambda: fastpitch.channel_project(h, lin.weight, lin.bias, n_dev), lambda: lin(h) * n_mask, g1),
           ("embed", lambda: fastpitch.scalar_embed(v, conv.weight, conv.bias, n_dev, h),
            lambda: (h + conv(v[:, None]).transpose(1, 2)) * n_mask, gd))
    for tag, nat, ref, g in ops:
        for side, fn in (("native", nat), ("torch", ref)):
            def fwd():
                with torch.no_grad():
                    fn()
            record("%s_%s_fwd" % (tag, side), fwd)
            record("%s_%s_fwd_bwd" % (tag, side), lambda: fn().backward(g))

    # one TemporalPredictor
    tp = fastpitch.TemporalPredictor(d, cfg.get("predictor_filter", 256), 3).to(dev)
    gp = torch.randn(B, N, device=dev)
    for side, fn in (("native", lambda: tp(h, n_dev)), ("torch", lambda: torch_predictor(tp, h, n_mask))):
        def fwd():
            with torch.no_grad():
                fn()
        record("predictor_%s_fwd" % side, fwd)
        record("predictor_%s_fwd_bwd" % side, lambda: fn().backward(gp))

    # the model: forward + backward under the loss, and infer
    model = fastpitch.FastPitch(cfg.pop("n_symbols", 148), **cfg).to(dev)
    with torch.no_grad():
        model.duration_predictor.fc.bias.fill_(1.6)                         # around 4 frames a token
    text = torch.randint(1, 11, (B, N), device=dev) * n_mask[:, :, 0].long()
    durations = (torch.randint(1, 8, (B, N), device=dev) * n_mask[:, :, 0].long()).to(torch.int32)
    T = int(durations.sum(dim=1).max())
    res["frames"] = int(durations.sum())
    target = torch.randn(B, T, model.n_mel, device=dev)
    loss = fastpitch.FastPitchLoss()

    def nat_fb():
        loss(model(text, durations, v, text_lengths=n_dev, max_frames=T), target, durations, v, None, n_dev)[0].backward()

    def ref_fb():
        loss(torch_model(model, text, durations, v, n_mask, T), target, durations, v, None, n_dev)[0].backward()
    record("model_native_fwd_bwd", nat_fb)
    record("model_torch_fwd_bwd", ref_fb)
    record("infer_native", lambda: model.infer(text, text_lengths=n_dev, max_frames=min(4096, 8 * N)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--smallest", action="store_true", help="one small case: the tool's own test")
    ap.add_argument("--out")
    a = ap.parse_args()
    small = dict(n_symbols=11, d_model=64, n_layer=2, n_head=1, d_head=32, d_inner=128, predictor_filter=64)
    if a.smallest:
        cases = [("smallest", 2, 12, small)]
    else:
        cases = [("b1_n187", 1, 187, {}), ("b16_ragged", 16, 187, {}), ("b64_tokens", 64, 160, {})]
    out = dict(tool="bench_fastpitch", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup,
               cases=[bench_case(n, B, N, dict(cfg), a.iters, min(a.warmup, a.iters)) for n, B, N, cfg in cases])
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
