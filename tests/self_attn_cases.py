"""The cases tests/test_self_attn_cpu.py (host stand-in) and tests/test_zz28_self_attn_gpu.py (MI355X) share for the masked
self-attention of DESIGN.md section 22: inputs, the two restatements of each case (computed once and kept), the harness that lays
a batch out with NaN in every utterance's padding and poisoned outputs, and the comparison under the project's tolerance."""
import functools

import numpy as np
import torch

import self_attn_ref as sr

# T_b at H = 1, D = 32: around the 32-row wave, the 64-key forward tile and the 128-row workgroup
SHAPES_D32 = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 257)
SHAPES_SUB = (1, 33, 65, 129, 257)
HEADS = ((2, 64), (3, 32), (1, 128))
KINDS = ("normal", "large")
PLANTED = ("first", "last", "rising")
TENSORS = ("o", "lse", "dq", "dk", "dv")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(T, H, D, kind="normal", seed=0):
    """One utterance: q, k, v, g (T, H, D) float32, the scale, and both restatements.  ``large`` scales q so that |s| reaches
    about 60; ``first`` / ``last`` / ``rising`` plant, in head 0, a row (t = T // 3) whose maximum lies in the first key tile, in
    the last, or in a strictly later tile after every tile of 64 keys, and a row (t = T // 2) of all-equal scores."""
    rs = np.random.RandomState(1000003 * T + 101 * H + D + 7 * seed + sum(map(ord, kind)))
    q, k, v, g = (rs.randn(T, H, D).astype(np.float32) for _ in range(4))
    scale = float(D) ** -0.5
    if kind == "large":
        s = scale * np.einsum("thd,jhd->htj", q.astype(np.float64), k.astype(np.float64))
        q = (q * np.float32(60.0 / max(np.abs(s).max(), 1e-3))).astype(np.float32)
    if kind in PLANTED:
        t0, t1 = T // 3, T // 2
        assert t0 != t1 and T > 64
        e = (q[t0, 0] / np.linalg.norm(q[t0, 0])).astype(np.float32)
        q[t0, 0] = np.float32(3.0 * np.sqrt(D)) * e                         # s(t0, j) = 3 (k_j . e): the planted part dominates
        tile = np.arange(T) // 64
        boost = {"first": np.where(np.arange(T) == 5, 8.0, 0.0), "last": np.where(np.arange(T) == T - 1, 8.0, 0.0),
                 "rising": 8.0 * (tile + 1.0)}[kind]
        k[:, 0] = k[:, 0] + boost[:, None].astype(np.float32) * e[None, :]
        q[t1, 0] = 0.0
        row = scale * (k[:, 0].astype(np.float64) @ q[t0, 0].astype(np.float64))
        best = np.array([row[j0:j0 + 64].max() for j0 in range(0, T, 64)])
        if kind == "first":
            assert best.argmax() == 0
        elif kind == "last":
            assert best.argmax() == len(best) - 1
        else:
            assert len(best) > 2 and np.all(np.diff(best) > 0)
    c = dict(T=T, H=H, D=D, kind=kind, q=q, k=k, v=v, g=g, scale=scale)
    c["f64"] = sr.attention64(q, k, v, g, scale)
    c["f32"] = sr.attention32(q, k, v, g, scale)
    for x in (q, k, v, g):
        x.setflags(write=False)
    return c


def _nan_buffer(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def layout(cases, dev, T=None, packed=False, offset=0):
    """q, k, v, g as (B, T, H, D) device views with NaN wherever no utterance has a frame.  ``packed``: q, k, v are the three
    chunks of one (B, T, 3 H D) buffer; otherwise each has a row of H D + 4 ``offset`` floats and starts 4 ``offset`` floats into
    its storage."""
    B, H, D = len(cases), cases[0]["H"], cases[0]["D"]
    T = max([c["T"] for c in cases] + [1]) if T is None else T
    if packed:
        buf = _nan_buffer((B, T, 3 * H * D), dev)
        views = [buf[:, :, i * H * D:(i + 1) * H * D].view(B, T, H, D) for i in range(3)]
        views.append(_nan_buffer((B, T, H, D), dev))
    else:
        views = []
        for _ in range(4):
            flat = _nan_buffer((4 * offset + B * T * (H * D + 4 * offset),), dev)
            views.append(flat[4 * offset:].view(B, T, H * D + 4 * offset)[:, :, :H * D].view(B, T, H, D))
    for b, c in enumerate(cases):
        for x, name in zip(views, ("q", "k", "v", "g")):
            if c["T"]:
                x[b, :c["T"]] = torch.from_numpy(np.array(c[name])).to(dev)
    lengths = torch.tensor([c["T"] for c in cases], dtype=torch.int32).to(dev)
    return views, lengths, T


def run(cases, dev, T=None, packed=False, offset=0, backward=True, scale=None):
    """The native calls on a batch of cases, outputs and workspace poisoned -> dict of numpy arrays (B, T, H, D) and (B, H, T)."""
    from tacotron2_amd import native as nv
    (q, k, v, g), lengths, T = layout(cases, dev, T, packed, offset)
    B, H, D = len(cases), cases[0]["H"], cases[0]["D"]
    scale = cases[0]["scale"] if scale is None else scale
    o, dq, dk, dv = (_nan_buffer((B, T, H, D), dev) for _ in range(4))
    lse = _nan_buffer((B, H, T), dev)
    nv.self_attn(q, k, v, lengths, scale, o, lse)
    out = dict(o=o, lse=lse)
    if backward:
        ws = torch.full((nv.self_attn_workspace(B, T, H, D, 2),), 0xFF, dtype=torch.uint8, device=dev)
        nv.self_attn_backward(q, k, v, o, lse, g, lengths, scale, dq, dk, dv, ws)
        out.update(dq=dq, dk=dk, dv=dv, delta=ws.view(torch.float32)[:B * H * T].view(B, H, T))
    return {n: x.cpu().numpy() for n, x in out.items()}


def region(name, x, b, T):
    """Utterance b's own part of an output, and the rest of its rows."""
    return (x[b, :, :T], x[b, :, T:]) if name in ("lse", "delta") else (x[b, :T], x[b, T:])


def check(c, out, b=0, label="", names=TENSORS):
    """Every tensor of utterance b against float64 under max(4 x the restatement's own error, 8 u max(1, |value|)); exact +0 in
    the padding.  -> {tensor: error / allowed}."""
    ratios = {}
    for n in names:
        got, pad = region(n, out[n], b, c["T"])
        assert not bits(pad).any(), (label, n, "the padding is not +0")
        if not c["T"]:
            continue
        assert np.isfinite(got).all(), (label, n)
        err, tol = sr.error(got, c["f64"][n]), sr.allowed(c["f32"][n], c["f64"][n])
        ratios[n] = err / tol
    print("FIGURE self_attn %sT %d H %d D %d %s: error / allowed %s"
          % (label, c["T"], c["H"], c["D"], c["kind"], " ".join("%s %.3f" % (n, r) for n, r in ratios.items())))
    for n, r in ratios.items():
        assert r <= 1.0, (label, c["T"], c["H"], c["D"], c["kind"], n, r)
    return ratios


def run_delta(cases, dev, offset=0):
    """t2amd_self_attn_delta_f32 alone on the float32 restatement's o -> delta (B, H, T), poisoned first."""
    from tacotron2_amd import native as nv
    (_, _, _, g), lengths, T = layout(cases, dev, offset=offset)
    B, H, D = len(cases), cases[0]["H"], cases[0]["D"]
    o = _nan_buffer((B, T, H, D), dev)
    for b, c in enumerate(cases):
        if c["T"]:
            o[b, :c["T"]] = torch.from_numpy(np.array(c["f32"]["o"])).to(dev)
    delta = _nan_buffer((B, H, T), dev)
    nv.self_attn_delta(g, o, lengths, delta)
    return delta.cpu().numpy()


def check_delta(cases, delta):
    for b, c in enumerate(cases):
        got, pad = region("delta", delta, b, c["T"])
        assert not bits(pad).any(), (b, "the padding is not +0")
        if c["T"]:
            assert np.array_equal(bits(got), bits(c["f32"]["delta"])), (b, c["T"], c["H"], c["D"])


RAGGED = (0, 1, 5, 64, 65, 130)


def empty_case(H, D):
    z = np.zeros((0, H, D), np.float32)
    return dict(T=0, H=H, D=D, kind="empty", q=z, k=z, v=z, g=z, scale=float(D) ** -0.5)


def ragged_cases(H=2, D=32):
    return [empty_case(H, D) if T == 0 else case(T, H, D, "normal", seed=3) for T in RAGGED]
