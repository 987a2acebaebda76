"""The cases the CPU and the GPU tests of the feed-forward Transformer block share: builders with their
float64 and float32 restatements (tests/fft_block_ref.py), runners that lay a ragged batch out with NaN beyond every utterance
and call the public functions on a device, and the checks under the project's tolerance
max(4 x the float32 restatement's own largest error, 8 2^-24 max(1, largest |value| in float64))."""
import numpy as np
import torch

import fft_block_ref as fr

F32 = np.float32
CONV_T_FIRST = (1, 2, 3, 4, 127, 128, 129, 257)
CONV_FIRST = (32, 64, 3)
CONV_T_SUB = (1, 5, 129)
CONV_SUB = ((64, 32, 1), (32, 160, 9), (96, 96, 5))
LN_C = (32, 36, 384, 4096)
LN_T = (1, 3, 65)
RAGGED = (0, 1, 2, 5, 128, 130)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


def conv_weights(Cin, Cout, k, bias, seed=0):
    r = np.random.default_rng(1000 + seed + Cin * 7 + Cout * 13 + k)
    w = (r.standard_normal((Cout, Cin, k)) / np.sqrt(Cin * k)).astype(F32)
    return w, (r.standard_normal(Cout).astype(F32) if bias else None)


def conv_batch(Ts, Cin, Cout, k, relu, bias, seed=0):
    """A batch of utterances under one weight: per utterance x, g and the float64 / float32 y and dx; for the batch dw and db."""
    w, b = conv_weights(Cin, Cout, k, bias, seed)
    r = np.random.default_rng(seed * 7919 + sum(Ts) + 31 * len(Ts) + Cin + k)
    utts = []
    for T in Ts:
        x, g = r.standard_normal((T, Cin)).astype(F32), r.standard_normal((T, Cout)).astype(F32)
        u = dict(T=T, x=x, g=g)
        if T:
            dx, dw, db = fr.conv_bwd64(x, w, b, relu, g)
            u["f64"] = dict(y=fr.conv64(x, w, b, relu), dx=dx, dw=dw, db=db)
            y32 = fr.conv32(x, w, b, relu)
            gm = fr.relu_mask32(g, y32) if relu else g
            u["f32"] = dict(y=y32, dx=fr.dx32(gm, w), gm=gm)
        utts.append(u)
    return dict(utts=utts, w=w, b=b, relu=relu, k=k, Cin=Cin, Cout=Cout)


def conv_batch_sums(batch, T_max):
    """The batch's dw and db in float64 and in the kernels' float32 order at the padded length ``T_max``."""
    live = [u for u in batch["utts"]]
    f64 = dict(dw=sum(u["f64"]["dw"] for u in live if u["T"]), db=sum(u["f64"]["db"] for u in live if u["T"]))
    gs = [u["f32"]["gm"] if u["T"] else np.zeros((0, batch["Cout"]), F32) for u in live]
    xs = [u["x"] for u in live]
    f32 = dict(dw=fr.dw32(gs, xs, batch["w"].shape, T_max), db=fr.colsum32(gs, T_max)[0])
    return f64, f32


def layout(arrays, dev, T, offset=0, wide=0):
    """The utterances' (T_b, C) arrays as one (B, T, C) device tensor with NaN beyond T_b; ``offset`` shifts the base by
    4 offset floats, ``wide`` adds 4 wide floats to every row's stride."""
    B, C = len(arrays), arrays[0].shape[1]
    buf = torch.full((4 * offset + B * T * (C + 4 * wide),), float("nan"), dtype=torch.float32)
    view = buf[4 * offset:].view(B, T, C + 4 * wide)[:, :, :C]
    for b, a in enumerate(arrays):
        view[b, :len(a)] = torch.from_numpy(np.ascontiguousarray(a))
    full = buf.to(dev)
    return full[4 * offset:].view(B, T, C + 4 * wide)[:, :, :C]


def run_conv(batch, dev, T=None, offset=0, wide=0, device_lengths=True):
    """ragged_conv1d forward and backward on the batch -> dict of numpy y, dx (B, T, .), dw, db."""
    from tacotron2_amd import transformer
    utts = batch["utts"]
    T = T or max(1, max(u["T"] for u in utts))
    x = layout([u["x"] for u in utts], dev, T, offset, wide).requires_grad_(True)
    g = layout([u["g"] for u in utts], dev, T, offset)
    w = torch.from_numpy(batch["w"]).to(dev).requires_grad_(True)
    b = None if batch["b"] is None else torch.from_numpy(batch["b"]).to(dev).requires_grad_(True)
    lens = [u["T"] for u in utts]
    lengths = torch.tensor(lens, dtype=torch.int32, device=dev) if device_lengths else lens
    y = transformer.ragged_conv1d(x, w, b, lengths, relu=batch["relu"])
    y.backward(g)
    out = dict(y=y.detach().cpu().numpy(), dx=x.grad.cpu().numpy(), dw=w.grad.cpu().numpy(), T=T)
    if b is not None:
        out["db"] = b.grad.cpu().numpy()
    return out


def check_conv(batch, out, label=""):
    """y and dx per utterance, dw and db for the batch, exact +0 in the padding; prints the FIGURE ratios."""
    worst = {}
    for bi, u in enumerate(batch["utts"]):
        T = u["T"]
        for n in ("y", "dx"):
            assert not bits(out[n][bi, T:]).any(), (label, bi, n, "padding")
            if T:
                ratio = fr.error(out[n][bi, :T], u["f64"][n]) / fr.allowed(u["f32"][n], u["f64"][n])
                worst[n] = max(worst.get(n, 0.0), ratio)
    f64, f32 = conv_batch_sums(batch, out["T"])
    for n in ("dw", "db"):
        if n in out:
            worst[n] = fr.error(out[n], f64[n]) / fr.allowed(f32[n], f64[n])
    print("FIGURE fft_block conv %s(Cin %d Cout %d k %d relu %d bias %d, frames %s): error / allowed %s"
          % (label, batch["Cin"], batch["Cout"], batch["k"], batch["relu"], batch["b"] is not None,
             ",".join(str(u["T"]) for u in batch["utts"][:8]), " ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst
    return worst


# ---- add + LayerNorm -----------------------------------------------------------------------------------------------------------
def ln_batch(Ts, C, residual, seed=0, plant=False, eps=1e-5):
    r = np.random.default_rng(seed * 104729 + sum(Ts) + 17 * len(Ts) + C)
    w, b = (1.0 + 0.1 * r.standard_normal(C)).astype(F32), (0.1 * r.standard_normal(C)).astype(F32)
    utts = []
    for T in Ts:
        x, g = r.standard_normal((T, C)).astype(F32), r.standard_normal((T, C)).astype(F32)
        res = r.standard_normal((T, C)).astype(F32) if residual else None
        if plant and T >= 1:                                                # a row of all-equal values: var = 0, y = bias
            x[0] = 0.75
            if res is not None:
                res[0] = 0.5
        if plant and T >= 2:                                                # |z| around 1e4 on a spread of 1
            x[1] = (1.0e4 + r.standard_normal(C)).astype(F32)
            if res is not None:
                res[1] = 0.0
        u = dict(T=T, x=x, g=g, res=res)
        if T:
            dz, dw, db = fr.add_ln_bwd64(x, res, w, eps, g)
            u["f64"] = dict(y=fr.add_ln64(x, res, w, b, eps), dz=dz, dw=dw, db=db)
            y, z, mean, rstd = fr.add_ln32(x, res, w, b, eps)
            dz32, xh = fr.add_ln_bwd32(g, z, mean, rstd, w)
            u["f32"] = dict(y=y, z=z, mean=mean, rstd=rstd, dz=dz32, xh=xh)
        utts.append(u)
    return dict(utts=utts, w=w, b=b, C=C, eps=eps, residual=residual)


def ln_batch_sums(batch, T_max):
    live = [u for u in batch["utts"] if u["T"]]
    f64 = dict(dw=sum(u["f64"]["dw"] for u in live), db=sum(u["f64"]["db"] for u in live))
    C = batch["C"]
    gs = [u["g"] if u["T"] else np.zeros((0, C), F32) for u in batch["utts"]]
    xhs = [u["f32"]["xh"] if u["T"] else np.zeros((0, C), F32) for u in batch["utts"]]
    db, dw = fr.colsum32(gs, T_max, xhs)
    return f64, dict(dw=dw, db=db)


def run_ln(batch, dev, T=None, offset=0, device_lengths=True):
    from tacotron2_amd import transformer
    utts = batch["utts"]
    T = T or max(1, max(u["T"] for u in utts))
    x = layout([u["x"] for u in utts], dev, T, offset).requires_grad_(True)
    res = layout([u["res"] for u in utts], dev, T, offset).requires_grad_(True) if batch["residual"] else None
    g = layout([u["g"] for u in utts], dev, T, offset)
    w, b = (torch.from_numpy(batch[n]).to(dev).requires_grad_(True) for n in ("w", "b"))
    lens = [u["T"] for u in utts]
    lengths = torch.tensor(lens, dtype=torch.int32, device=dev) if device_lengths else lens
    y = transformer.add_layer_norm(x, res, w, b, lengths, batch["eps"])
    y.backward(g)
    out = dict(y=y.detach().cpu().numpy(), dz=x.grad.cpu().numpy(), dw=w.grad.cpu().numpy(), db=b.grad.cpu().numpy(), T=T)
    if res is not None:
        out["dres"] = res.grad.cpu().numpy()
    return out


def check_ln(batch, out, label="", exact=False):
    """Under the tolerance, or with ``exact`` bit for bit against the float32 restatement (the host stand-in)."""
    worst = {}
    f64, f32 = ln_batch_sums(batch, out["T"])
    for bi, u in enumerate(batch["utts"]):
        T = u["T"]
        for n in ("y", "dz"):
            assert not bits(out[n][bi, T:]).any(), (label, bi, n, "padding")
            if not T:
                continue
            if exact:
                assert np.array_equal(bits(out[n][bi, :T]), bits(u["f32"][n])), (label, bi, n)
            worst[n] = max(worst.get(n, 0.0), fr.error(out[n][bi, :T], u["f64"][n]) / fr.allowed(u["f32"][n], u["f64"][n]))
        if "dres" in out:
            assert np.array_equal(bits(out["dres"]), bits(out["dz"])), (label, "dres")
    for n in ("dw", "db"):
        if exact:
            assert np.array_equal(bits(out[n]), bits(f32[n])), (label, n)
        worst[n] = fr.error(out[n], f64[n]) / fr.allowed(f32[n], f64[n])
    print("FIGURE fft_block add_ln %s(C %d residual %d, frames %s): error / allowed %s"
          % (label, batch["C"], batch["residual"], ",".join(str(u["T"]) for u in batch["utts"][:8]),
             " ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst
    return worst


# ---- the modules in torch, one utterance alone ---------------------------------------------------------------------------------
def conv_ff_ref(sd, prefix, x, ks, pre):
    """PositionwiseConvFF on one utterance (T, d) from the state dict, in x's dtype."""
    F = torch.nn.functional
    p = lambda n: sd[prefix + n].to(x.dtype)                                # noqa: E731
    ln = lambda v: F.layer_norm(v, (v.shape[1],), p("layer_norm.weight"), p("layer_norm.bias"), 1e-5)  # noqa: E731
    h = ln(x) if pre else x
    h = F.relu(F.conv1d(h.t()[None], p("conv1.weight"), p("conv1.bias"), padding=ks[0] // 2))
    h = F.conv1d(h, p("conv2.weight"), p("conv2.bias"), padding=ks[1] // 2)[0].t()
    return h + x if pre else ln(h + x)


def attn_ref(sd, prefix, x, n_head, d_head, pre):
    F = torch.nn.functional
    p = lambda n: sd[prefix + n].to(x.dtype)                                # noqa: E731
    ln = lambda v: F.layer_norm(v, (v.shape[1],), p("layer_norm.weight"), p("layer_norm.bias"), 1e-5)  # noqa: E731
    T = x.shape[0]
    h = ln(x) if pre else x
    q, k, v = (c.view(T, n_head, d_head).transpose(0, 1) for c in F.linear(h, p("qkv_net.weight"), p("qkv_net.bias")).chunk(3, dim=1))
    a = torch.softmax(q @ k.transpose(1, 2) * d_head ** -0.5, dim=2) @ v
    out = x + F.linear(a.transpose(0, 1).reshape(T, n_head * d_head), p("o_net.weight"))
    return out if pre else ln(out)


def block_ref(sd, prefix, x, n_head, d_head, ks, pre):
    return conv_ff_ref(sd, prefix + "pos_ff.", attn_ref(sd, prefix + "dec_attn.", x, n_head, d_head, pre), ks, pre)


def pos_emb_ref(T, d, dtype=torch.float64):
    pos = torch.arange(T, dtype=dtype)[:, None]
    f = 10000.0 ** (-torch.arange(0, d, 2, dtype=dtype) / d)
    return torch.cat([torch.sin(pos * f), torch.cos(pos * f)], dim=1)
