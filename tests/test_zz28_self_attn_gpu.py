"""Masked multi-head self-attention on the MI355X (transformer.self_attention, transformer.MultiHeadSelfAttention,
csrc/self_attn.hip, csrc/self_attn_rows.hip, tools/bench_self_attn.py) against the float64 restatement (tests/self_attn_ref.py).

Per case and per tensor (o, lse, dq, dk, dv) the largest absolute error over the utterance's region is at most
max(4 x the float32 restatement's own largest error on that case, 8 2^-24 max(1, largest |value| of that tensor in float64))
(DESIGN.md sections 19.4 / 20.4 / 22.4).  Every case prints its ratios error / allowed (``FIGURE`` lines;
profiles/self_attn_pytest_gpu.txt has the run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
import self_attn_cases as sc
import self_attn_ref as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("T", sc.SHAPES_D32)
def test_shapes_one_head_of_32(native_lib, T, kind):
    c = sc.case(T, 1, 32, kind)
    sc.check(c, sc.run([c], DEV, T=T + T % 3, offset=T % 2))


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("T", sc.SHAPES_SUB)
@pytest.mark.parametrize("heads", sc.HEADS)
def test_shapes_more_heads_and_wider_heads(native_lib, heads, T, kind):
    c = sc.case(T, heads[0], heads[1], kind)
    sc.check(c, sc.run([c], DEV, T=T + T % 2, packed=bool(T % 3)))


@pytest.mark.parametrize("kind", sc.PLANTED)
def test_planted_row_maxima_and_a_row_of_equal_scores(native_lib, kind):
    """The row t = T // 3 of head 0 has its maximum in the first key tile, in the last, or in a strictly later tile after every
    tile (every step rescales); the row t = T // 2 has all-equal scores: its o is the mean of v and its lse log T."""
    c = sc.case(257, 1, 32, kind)
    out = sc.run([c], DEV)
    sc.check(c, out, label="planted ")
    t1 = 257 // 2
    assert np.abs(out["o"][0, t1, 0] - c["v"][:, 0].astype(np.float64).mean(axis=0)).max() <= 8 * sr.U * 257 ** 0.5
    assert abs(out["lse"][0, 0, t1] - np.log(257.0)) <= 8 * sr.U * np.log(257.0)


def test_two_long_utterances(native_lib):
    cases = [sc.case(870, 2, 64), sc.case(500, 2, 64)]
    out = sc.run(cases, DEV, packed=True)
    for b, c in enumerate(cases):
        sc.check(c, out, b, label="B 2 ")


def test_the_frame_limit(native_lib):
    c = sc.case(4096, 1, 32)
    sc.check(c, sc.run([c], DEV), label="limit ")


def test_ragged_batch_equals_each_utterance_alone_and_two_calls_agree(native_lib):
    """Six utterances (0, 1, 5, 64, 65, 130 frames) with NaN beyond T_b in q, k, v and g: exact zeros in the padding, the same
    bits as each utterance alone at another stride and offset, the same bits from a second call, and the chunks of a packed
    projection the same bits as contiguous copies."""
    cases = sc.ragged_cases()
    batch = sc.run(cases, DEV, T=131)
    again = sc.run(cases, DEV, T=131)
    packed = sc.run(cases, DEV, T=131, packed=True)
    for n in sc.TENSORS + ("delta",):
        assert np.array_equal(sc.bits(batch[n]), sc.bits(again[n])), n
        assert np.array_equal(sc.bits(batch[n]), sc.bits(packed[n])), n
    for b, c in enumerate(cases):
        sc.check(c, batch, b, label="ragged ")
        if c["T"]:
            alone = sc.run([c], DEV, T=c["T"] + b % 2, offset=1 + b % 3)
            for n in sc.TENSORS:
                assert np.array_equal(sc.bits(sc.region(n, batch[n], b, c["T"])[0]), sc.bits(sc.region(n, alone[n], 0, c["T"])[0])), (b, n)


def test_more_utterances_than_compute_units(native_lib):
    cases = [sc.case(1 + i % 11, 1, 32, "normal", seed=i // 11) for i in range(300)]
    out = sc.run(cases, DEV)
    worst = {}
    for b, c in enumerate(cases):
        for n in sc.TENSORS:
            got, pad = sc.region(n, out[n], b, c["T"])
            assert not sc.bits(pad).any(), (b, n)
            worst[n] = max(worst.get(n, 0.0), sr.error(got, c["f64"][n]) / sr.allowed(c["f32"][n], c["f64"][n]))
    print("FIGURE self_attn 300 utterances of 1 to 11 frames: error / allowed %s" % " ".join("%s %.3f" % kv for kv in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_autograd_with_a_random_and_an_expanded_gradient(native_lib):
    from tacotron2_amd import transformer
    cases = sc.ragged_cases()
    want = sc.run(cases, DEV, T=131)
    (q, k, v, g), lengths, T = sc.layout(cases, DEV, T=131)
    leaves = [x.detach().clone().requires_grad_(True) for x in (q, k, v)]
    o = transformer.self_attention(*leaves, lengths)
    assert o.grad_fn is not None and np.array_equal(sc.bits(o.detach().cpu().numpy()), sc.bits(want["o"]))
    o.backward(g)
    for leaf, n in zip(leaves, ("dq", "dk", "dv")):
        assert leaf.grad.is_contiguous() and np.array_equal(sc.bits(leaf.grad.cpu().numpy()), sc.bits(want[n])), n
    with torch.no_grad():
        plain = transformer.self_attention(*leaves, [c["T"] for c in cases])
    assert plain.grad_fn is None and torch.equal(plain, o.detach())
    assert transformer.self_attention(q, k, v, lengths).grad_fn is None
    # the expanded gradient of .sum().backward() is copied; (T, H, D) is a batch of one; only v needs a gradient
    c = cases[5]
    ones = dict(c, g=np.ones_like(c["g"]))
    ref = sr.attention64(c["q"], c["k"], c["v"], ones["g"], c["scale"])
    ref32 = sr.attention32(c["q"], c["k"], c["v"], ones["g"], c["scale"])
    q1, k1, v1 = (torch.from_numpy(np.array(c[n])).to(DEV) for n in ("q", "k", "v"))
    v1.requires_grad_(True)
    one = transformer.self_attention(q1, k1, v1)
    assert tuple(one.shape) == (1, c["T"], c["H"], c["D"])
    one.sum().backward()
    assert sr.error(v1.grad.cpu().numpy(), ref["dv"]) <= sr.allowed(ref32["dv"], ref["dv"])
    # a scale of the caller's
    c2 = sc.case(33, 2, 32)
    got = transformer.self_attention(*(torch.from_numpy(np.array(c2[n])).to(DEV) for n in ("q", "k", "v")), scale=0.5)
    f64 = sr.attention64(c2["q"], c2["k"], c2["v"], c2["g"], 0.5)["o"]
    assert sr.error(got.cpu().numpy()[0], f64) <= sr.allowed(sr.attention32(c2["q"], c2["k"], c2["v"], c2["g"], 0.5)["o"], f64)


def test_device_lengths_make_no_device_to_host_copy(native_lib):
    from tacotron2_amd import transformer
    cases = sc.ragged_cases()
    (q, k, v, g), lengths, T = sc.layout(cases, DEV, T=131, packed=True)
    leaves = [x.detach().clone().requires_grad_(True) for x in (q, k, v)]
    mod = transformer.MultiHeadSelfAttention(2, 48, 32).to(DEV)
    x = torch.randn(len(cases), T, 48, device=DEV)
    long_lengths = lengths.long()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        transformer.self_attention(*leaves, lengths).backward(g)
        with torch.no_grad():
            transformer.self_attention(q, k, v, long_lengths)
        mod(x, lengths).sum().backward()
        with pytest.raises(RuntimeError, match="synchroniz"):
            lengths.tolist()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(leaf.grad is not None for leaf in leaves) and mod.qkv_net.weight.grad is not None


def test_module_equals_a_float64_torch_restatement(native_lib):
    from tacotron2_amd import transformer
    B, T, H, D, M = 3, 70, 2, 32, 48
    lens = [70, 1, 37]
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(B, T, M, generator=gen)
    gy = torch.randn(B, T, M, generator=gen)
    live = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None])
    for pre in (False, True):
        torch.manual_seed(5)
        mod = transformer.MultiHeadSelfAttention(H, M, D, pre_lnorm=pre)
        ref = transformer.MultiHeadSelfAttention(H, M, D, pre_lnorm=pre).double()
        ref.load_state_dict(mod.state_dict())
        x64 = x.double().requires_grad_(True)
        h = ref.layer_norm(x64) if pre else x64
        q, k, v = (c.view(B, T, H, D) for c in ref.qkv_net(h).chunk(3, dim=2))
        s = (D ** -0.5) * torch.einsum("bthd,bjhd->bhtj", q, k)
        p = torch.softmax(s.masked_fill(~live[:, None, None, :], float("-inf")), dim=3)
        o = torch.einsum("bhtj,bjhd->bthd", p, v) * live[:, :, None, None]
        y64 = x64 + ref.o_net(o.reshape(B, T, H * D))
        y64 = y64 if pre else ref.layer_norm(y64)
        (y64 * gy.double()).sum().backward()
        mod = mod.to(DEV)
        xd = x.to(DEV).requires_grad_(True)
        y = mod(xd, lens)
        (y * gy.to(DEV)).sum().backward()
        tol = lambda r: 64 * sr.U * max(1.0, float(r.detach().abs().max())) * (T + M) ** 0.5          # noqa: E731
        assert float((y.detach().cpu().double() - y64.detach()).abs().max()) <= tol(y64), pre
        assert float((xd.grad.cpu().double() - x64.grad).abs().max()) <= tol(x64.grad), pre
        for (n, a), (_, b) in zip(mod.named_parameters(), ref.named_parameters()):
            assert float((a.grad.cpu().double() - b.grad).abs().max()) <= tol(b.grad), (pre, n)
        # the rows beyond an utterance's frames are what the residual path gives
        pad = x.to(DEV) + 0.0 if pre else mod.layer_norm(x.to(DEV))
        assert torch.equal(y.detach()[1, 1:], pad.detach()[1, 1:])


def test_refusals_on_the_device(native_lib):
    from tacotron2_amd import native, transformer
    f = transformer.self_attention
    q = torch.zeros(2, 6, 2, 32, device=DEV)
    with pytest.raises(ValueError, match="self_attention: q is on cuda:0 and k on cpu"):
        f(q, q.cpu(), q)
    with pytest.raises(ValueError, match="self_attention: q is on cpu and v on cuda:0"):
        f(q.cpu(), q.cpu(), q)
    with pytest.raises(native.NativeError, match="self_attention: q, k and v are on cpu.*no CPU path"):
        f(q.cpu(), q.cpu(), q.cpu())
    with pytest.raises(TypeError, match="self_attention: expected float32 q, got torch.float16"):
        f(q.half(), q, q)
    with pytest.raises(TypeError, match="self_attention: expected float32 k, got torch.bfloat16"):
        f(q, q.bfloat16(), q)
    with pytest.raises(ValueError, match="self_attention: a head width of 48 is not one of 32, 64, 96, 128"):
        f(*(torch.zeros(1, 4, 1, 48, device=DEV),) * 3)
    with pytest.raises(ValueError, match="self_attention: 17 heads exceed the limit of 16"):
        f(*(torch.zeros(1, 4, 17, 32, device=DEV),) * 3)
    with pytest.raises(ValueError, match="self_attention: 4097 frames exceed the limit of 4096"):
        f(*(torch.zeros(1, 4097, 1, 32, device=DEV),) * 3)
    with pytest.raises(ValueError, match=r"self_attention: utterance 1: 7 frames do not lie in \[0, 6\]"):
        f(q, q, q, [6, 7])
    with pytest.raises(ValueError, match="self_attention: expected 2 integer lengths"):
        f(q, q, q, torch.tensor([6, 6, 6], device=DEV))
    with pytest.raises(ValueError, match="self_attention: expected 2 integer lengths"):
        f(q, q, q, torch.tensor([6.0, 6.0], device=DEV))
    # device lengths beyond [0, T] are clamped, not refused
    r = torch.randn(2, 6, 2, 32, device=DEV)
    assert torch.equal(f(r, r, r, torch.tensor([9, -3], device=DEV)), f(r, r, r, [6, 0]))
    # a tensor the kernels cannot read as it is, is copied: a transposed one, and one that starts 4 bytes into its storage
    odd = torch.randn(2 * 6 * 2 * 32 + 1, device=DEV)[1:].view(2, 6, 2, 32)
    assert odd.data_ptr() % 16 and torch.equal(f(odd, odd, odd), f(odd.clone(), odd.clone(), odd.clone()))
    tr = r.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not tr.is_contiguous() and torch.equal(f(tr, r, r), f(r, r, r))


def test_memory(native_lib):
    """Forward + backward at B = 4, H = 2, T = 1024, D = 64: the peak above the baseline, less the bytes of the inputs, outputs
    and gradients the call returns or keeps (o, dq, dk, dv: four tensors of the inputs' size), stays below one (B, H, T, T)
    float32 matrix (33.5 MB); under no_grad it is what t2amd_self_attn_workspace reports for the forward (nothing) beside o."""
    from tacotron2_amd import native, transformer
    B, H, T, D = 4, 2, 1024, 64
    gen = torch.Generator().manual_seed(1)
    q, k, v, g = (torch.randn(B, T, H, D, generator=gen).to(DEV) for _ in range(4))
    lens = torch.tensor([1024, 700, 1000, 3], dtype=torch.int32).to(DEV)
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
    one = 4 * B * T * H * D
    transformer.self_attention(*leaves, lens).backward(g)                   # warm-up: the library and the allocator
    for leaf in leaves:
        leaf.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    o = transformer.self_attention(*leaves, lens)
    o.backward(g)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base - 4 * one
    print("FIGURE self_attn memory: forward + backward peak above inputs, outputs and gradients %d bytes; one score matrix %d bytes"
          % (extra, 4 * B * H * T * T))
    assert native.self_attn_workspace(B, T, H, D, 1) + native.self_attn_workspace(B, T, H, D, 2) <= extra < 4 * B * H * T * T
    del o
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        o = transformer.self_attention(q, k, v, lens)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base - one == native.self_attn_workspace(B, T, H, D, 0) == 0


def test_bench_tool_at_its_smallest_case(native_lib, tmp_path):
    out = tmp_path / "bench.json"
    r = subprocess.run([sys.executable, os.path.join(gu.ROOT, "tools", "bench_self_attn.py"), "--cases", "tiny", "--reps", "1", "--inner", "2",
                        "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == json.loads(out.read_text()) and set(res["cases"]) == {"tiny"}
    c = res["cases"]["tiny"]
    assert max(c["error_over_allowed"].values()) <= 1.0 and all(v > 0 for v in c["call_ms"].values())
    assert set(c["kernel_ms"]) == {"self_attn_fwd_kernel", "self_attn_delta_kernel", "self_attn_backward_three_kernels"}
    for name in ("torch_float32_bmm_softmax_bmm", "torch_scaled_dot_product_attention"):
        assert c[name]["forward_backward_ms"] > 0 and c[name]["max_abs_difference_of_o"] < 1e-4
