"""The feed-forward Transformer block's convolutional feed-forward and add + LayerNorm on the MI355X (transformer.ragged_conv1d,
transformer.add_layer_norm, PositionwiseConvFF, FFTBlock, FFTransformer, csrc/fft_block.hip, csrc/fft_block_rows.hip) against the
float64 restatement (tests/fft_block_ref.py).

Per case and per tensor the largest absolute error over the utterance's region is at most
max(4 x the float32 restatement's own largest error on that case, 8 2^-24 max(1, largest |value| of that tensor in float64))
(DESIGN.md sections 19.4 / 20.4 / 22.4 / 23.4).  Every case prints its ratios error / allowed (``FIGURE`` lines;
profiles/fft_block_pytest_gpu.txt has the run)."""
import numpy as np
import pytest
import torch

import fft_block_cases as fc
import fft_block_ref as fr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("T", fc.CONV_T_FIRST)
def test_conv_shapes_32_to_64_channels_3_taps(native_lib, T, relu, bias):
    batch = fc.conv_batch((T,), *fc.CONV_FIRST, relu, bias)
    fc.check_conv(batch, fc.run_conv(batch, DEV, T=T + 1 + T % 3, offset=1 + T % 2, wide=T % 2))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("T", fc.CONV_T_SUB)
@pytest.mark.parametrize("shape", fc.CONV_SUB)
def test_conv_shapes_other_widths_and_taps(native_lib, shape, T, relu, bias):
    batch = fc.conv_batch((T,), *shape, relu, bias)
    fc.check_conv(batch, fc.run_conv(batch, DEV, T=T + 2, offset=T % 3, wide=1))


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("T", fc.LN_T)
@pytest.mark.parametrize("C", fc.LN_C)
def test_add_layer_norm_shapes_with_planted_rows(native_lib, C, T, residual):
    """Row 0 holds all-equal values (var = 0: y = bias), row 1 |z| around 1e4 on a spread of 1."""
    batch = fc.ln_batch((T,), C, residual, plant=True)
    out = fc.run_ln(batch, DEV, T=T + 1, offset=T % 2)
    fc.check_ln(batch, out)
    assert np.array_equal(fc.bits(out["y"][0, 0]), fc.bits(batch["b"]))


def test_ragged_batch_equals_each_utterance_alone_and_two_calls_agree(native_lib):
    """Six utterances of (0, 1, 2, 5, 128, 130) frames with NaN beyond T_b in x, residual and g: exact +0 in the padding (inside
    the checks), the bits of each utterance alone at another T and base offset, and the same bits from a second call."""
    conv = fc.conv_batch(fc.RAGGED, 32, 160, 3, True, True)
    ln = fc.ln_batch(fc.RAGGED, 384, True)
    for batch, run, check, per_row in ((conv, fc.run_conv, fc.check_conv, ("y", "dx")), (ln, fc.run_ln, fc.check_ln, ("y", "dz"))):
        first, again = run(batch, DEV, T=131), run(batch, DEV, T=131)
        check(batch, first, "ragged ")
        for n in first:
            if n != "T":
                assert np.array_equal(fc.bits(first[n]), fc.bits(again[n])), n
        for b, u in enumerate(batch["utts"]):
            if u["T"]:
                alone = run(dict(batch, utts=[u]), DEV, T=u["T"] + b % 2, offset=1 + b % 3)
                for n in per_row:
                    assert np.array_equal(fc.bits(first[n][b, :u["T"]]), fc.bits(alone[n][0, :u["T"]])), (b, n)


def test_dw_across_many_short_utterances(native_lib):
    """300 utterances of 1 to 11 frames: a reduction of 9600 indices in 8 slices."""
    batch = fc.conv_batch(tuple(1 + i % 11 for i in range(300)), 32, 32, 3, True, True)
    assert fr.dw_plan(300, 11) == (32, 8, 1216)
    fc.check_conv(batch, fc.run_conv(batch, DEV), "300 utterances ")


def test_the_mask_epilogue_equals_the_separate_mask_pass(native_lib):
    """dx of the layer below a ReLU: the convolution's third epilogue keeps a value only where the second tensor is positive."""
    from tacotron2_amd import native
    batch = fc.conv_batch((5, 130), 32, 64, 3, False, False)
    T = 131
    g = fc.layout([u["g"] for u in batch["utts"]], DEV, T)
    act = fc.layout([u["x"] for u in batch["utts"]], DEV, T).contiguous()
    lens = torch.tensor([5, 130], dtype=torch.int32, device=DEV)
    image = torch.from_numpy(fr.image_dx(batch["w"])).to(DEV)
    plain, masked, want = (torch.empty(2, T, 32, device=DEV) for _ in range(3))
    native.ffb_conv(g, image, None, None, lens, 3, False, plain)
    native.ffb_conv(g, image, None, act, lens, 3, False, masked)
    native.ffb_relu_mask(plain, act, lens, want)
    assert torch.equal(masked.view(torch.int32), want.view(torch.int32)) and masked.abs().sum() > 0


# ---- the modules ---------------------------------------------------------------------------------------------------------------
MOD_T = (7, 33, 130)


def _module_check(module, ref_fn, label, ids=None):
    """The module on a ragged batch of (7, 33, 130) frames against the float64 torch run of the same formulation on each utterance
    alone, loaded from the state dict; the float32 torch run of the same is the restatement of the tolerance.  Output and every
    parameter gradient."""
    torch.manual_seed(11)
    module = module.to(DEV)
    with torch.no_grad():
        for p in module.parameters():
            p.add_(0.05 * torch.randn_like(p))
    sd = {k: v.detach().cpu() for k, v in module.state_dict().items()}
    r = np.random.default_rng(7)
    T, d = 131, 64
    xs = [r.standard_normal((t, d)).astype(F32) for t in MOD_T] if ids is None else [r.integers(1, 10, (t,)) for t in MOD_T]
    gs = [r.standard_normal((t, d)).astype(F32) for t in MOD_T]
    if ids is None:
        x = fc.layout(xs, DEV, T)
    else:
        x = torch.zeros(3, T, dtype=torch.long)
        for b, a in enumerate(xs):
            x[b, :len(a)] = torch.from_numpy(a)
        x = x.to(DEV)
    lengths = torch.tensor(MOD_T, dtype=torch.int32, device=DEV)
    out = module(x, lengths)
    out = out[0] if isinstance(out, tuple) else out
    assert not out.detach()[0, 7:].view(torch.int32).any() and not out.detach()[2, 130:].view(torch.int32).any()
    out.backward(fc.layout(gs, DEV, T))
    got = dict(out=[out.detach()[b, :t].cpu().numpy() for b, t in enumerate(MOD_T)])
    got.update({n: p.grad.cpu().numpy() for n, p in module.named_parameters()})
    refs = {}
    for dtype in (torch.float64, torch.float32):
        leaves = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
        outs = [ref_fn(leaves, torch.from_numpy(a) if ids is not None else torch.from_numpy(a).to(dtype)) for a in xs]
        sum((o * torch.from_numpy(g).to(dtype)).sum() for o, g in zip(outs, gs)).backward()
        refs[dtype] = dict(out=[o.detach().numpy() for o in outs])
        refs[dtype].update({n: leaves[n].grad.numpy() for n, _ in module.named_parameters()})
    worst = {}
    for n in got:
        pairs = zip(got[n], refs[torch.float32][n], refs[torch.float64][n]) if n == "out" else [(got[n], refs[torch.float32][n], refs[torch.float64][n])]
        for a, f32, f64 in pairs:
            worst[n] = max(worst.get(n, 0.0), fr.error(a, f64) / fr.allowed(f32, f64))
    print("FIGURE fft_block module %s: error / allowed %s" % (label, " ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("ks", [3, (9, 1)])
def test_positionwise_conv_ff(native_lib, ks, pre):
    from tacotron2_amd import transformer
    pair = (ks, ks) if isinstance(ks, int) else ks
    _module_check(transformer.PositionwiseConvFF(64, 128, ks, pre_lnorm=pre), lambda sd, x: fc.conv_ff_ref(sd, "", x, pair, pre),
                  "PositionwiseConvFF k %s pre %d" % (ks, pre))


@pytest.mark.parametrize("pre", [False, True])
def test_fft_block(native_lib, pre):
    from tacotron2_amd import transformer
    _module_check(transformer.FFTBlock(2, 64, 32, 128, 3, pre_lnorm=pre), lambda sd, x: fc.block_ref(sd, "", x, 2, 32, (3, 3), pre),
                  "FFTBlock pre %d" % pre)


def test_fft_transformer_with_an_embedding(native_lib):
    from tacotron2_amd import transformer

    def ref(sd, ids):
        h = sd["word_emb.weight"][ids]
        h = h + fc.pos_emb_ref(len(ids), 64, h.dtype)
        for i in range(2):
            h = fc.block_ref(sd, "layers.%d." % i, h, 2, 32, (3, 3), False)
        return h
    _module_check(transformer.FFTransformer(2, 2, 64, 32, 128, 3, n_embed=10), ref, "FFTransformer 2 layers", ids=True)


def test_positional_embedding_closed_form(native_lib):
    from tacotron2_amd import transformer
    lens = torch.tensor([3, 131], dtype=torch.int32, device=DEV)
    pe = transformer.positional_embedding(131, 64, lens, DEV).cpu()
    want = fc.pos_emb_ref(131, 64)
    # sin and cos of an argument up to 130 rounded to float32: u 130 of argument error, and the functions' own u
    assert (pe[1].double() - want).abs().max() <= 2 * fr.U * 131
    assert not pe[0, 3:].view(torch.int32).any() and torch.equal(pe[0, :3], pe[1, :3])


def test_no_host_copies_with_device_lengths(native_lib):
    from tacotron2_amd import transformer
    ff = transformer.PositionwiseConvFF(64, 128, 3).to(DEV)
    x = torch.randn(3, 40, 64, device=DEV, requires_grad=True)
    g = torch.randn(3, 40, 64, device=DEV)
    lengths = torch.tensor([40, 7, 0], dtype=torch.int32, device=DEV)
    ff(x, lengths).backward(g)                                              # warm: the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ff(x, lengths).backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_peak_memory_of_positionwise_conv_ff(native_lib):
    """forward + backward of the post-norm form, above x, g and the parameters, holds the output y, the parameter
    gradients and conv1's output h1 throughout, and peaks in one of the three backward nodes: add + LayerNorm's (its kept z, mean
    and rstd, dz, the column sums' workspace), conv2's (dz, dh1, the dx weight image, the dw workspace) or conv1's (dh1, its
    masked copy, dx, the image, the workspaces); the residual's gradient waits in x.grad through both convolutions' nodes.  The
    allocator rounds every tensor up to 512 bytes, hence 256 KiB of slack on a figure of 3.2 MiB."""
    from tacotron2_amd import native, transformer
    B, T, d, di, k = 4, 256, 64, 128, 3
    ff = transformer.PositionwiseConvFF(d, di, k).to(DEV)
    x = torch.randn(B, T, d, device=DEV, requires_grad=True)
    g = torch.randn(B, T, d, device=DEV)
    lengths = torch.tensor([256, 200, 31, 0], dtype=torch.int32, device=DEV)
    ff(x, lengths).backward(g)
    ff.zero_grad()
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = ff(x, lengths)
    y.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    act_d, act_i = 4 * B * T * d, 4 * B * T * di
    params = sum(4 * p.numel() for p in ff.parameters())
    image = 4 * d * di * k
    ws = native.fft_block_workspace
    ln_bwd = 2 * act_d + 8 * B * T + ws(B, T, d, d, 1, 2)                   # z, dz, mean and rstd, the partial sums
    conv2_bwd = 2 * act_d + act_i + image + ws(B, T, di, d, k, 1)           # dz, the residual's copy of it in x.grad, dh1
    conv1_bwd = 2 * act_i + 2 * act_d + image + ws(B, T, d, di, k, 1) + ws(B, T, di, di, 1, 2)   # dh1, masked, x.grad, dx
    derived = act_d + params + act_i + max(ln_bwd, conv2_bwd, conv1_bwd)
    print("FIGURE fft_block memory: peak %d bytes, derived %d bytes" % (peak, derived))
    assert derived // 2 <= peak <= derived + (1 << 18), (peak, derived)


def test_bench_tool_smallest_case(native_lib):
    import json
    import os
    import subprocess
    import sys
    import golden_util as gu
    out = subprocess.run([sys.executable, os.path.join(gu.ROOT, "tools", "bench_fft_block.py"), "--smallest", "--iters", "2"],
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["cases"] and all(c["native_fwd_ms"] > 0 and c["torch_fwd_ms"] > 0 for c in res["cases"])
