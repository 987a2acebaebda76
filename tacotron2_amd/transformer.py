"""Masked multi-head self-attention on the GPU (csrc/self_attn.hip, csrc/self_attn_rows.hip): the middle of
the feed-forward Transformer block of FastSpeech, FastPitch and FastSpeech 2, over a ragged batch.

    o = self_attention(q, k, v, lengths=None, scale=None)                   # (B, T, H, D), differentiable once
    y = MultiHeadSelfAttention(n_head, d_model, d_head, pre_lnorm=False)(x, lengths)

Per utterance b with T_b = lengths[b] frames and per head: p(t, .) = softmax over j < T_b of scale q(t, .) . k(j, .), o(t, :) =
sum_j p(t, j) v(j, :) for t < T_b and exactly +0 from there on.  A fused kernel pair on the exact-f32 matrix pipe: the forward
keeps a running maximum and sum per row, the backward recomputes the probabilities from the kept logsumexp, so no (T, T) matrix
exists in memory.  Exact f32 products, every sum in a fixed ascending order, no atomics: two calls give the same bits, and an
utterance in a ragged batch gives the bits it gives alone.  What lies at and beyond T_b in q, k, v and the gradient is never
read.  There is no CPU path."""
import math

import torch

from . import native as nv
from .audio import _lengths

MAX_FRAMES = 4096
MAX_HEADS = 16
MIN_HEAD_WIDTH = 32
MAX_HEAD_WIDTH = 128
MAX_BATCH_HEADS = 65535


def _as_operand(x):
    """``x`` (B, T, H, D) as the kernels take it: unit stride along D, the other strides positive multiples of 4 floats, the base
    on 16 bytes.  The chunks of a packed (B, T, 3 H D) projection pass as they are; anything else is copied."""
    ok = x.stride(3) == 1 and all(x.shape[i] == 1 or (x.stride(i) > 0 and x.stride(i) % 4 == 0) for i in range(3))
    if not ok:
        x = x.contiguous()
    return x if x.data_ptr() % 16 == 0 else x.clone(memory_format=torch.contiguous_format)


class _SelfAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, len_dev, scale, keep):
        B, T, H, D = q.shape
        dev = q.device
        qd, kd, vd = (_as_operand(t.detach()) for t in (q, k, v))
        o = torch.empty(B, T, H, D, dtype=torch.float32, device=dev)
        lse = torch.empty(B, H, T, dtype=torch.float32, device=dev) if keep else None
        nv.self_attn(qd, kd, vd, len_dev, scale, o, lse)
        if keep:
            ctx.scale, ctx.has_len = scale, len_dev is not None
            ctx.save_for_backward(qd, kd, vd, o, lse, *(() if len_dev is None else (len_dev,)))
        return o

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        q, k, v, o, lse = ctx.saved_tensors[:5]
        len_dev = ctx.saved_tensors[5] if ctx.has_len else None
        B, T, H, D = q.shape
        g = _as_operand(grad.float())
        dq, dk, dv = (torch.empty(B, T, H, D, dtype=torch.float32, device=q.device) for _ in range(3))
        ws = torch.empty(nv.self_attn_workspace(B, T, H, D, 2), dtype=torch.uint8, device=q.device)
        nv.self_attn_backward(q, k, v, o, lse, g, len_dev, ctx.scale, dq, dk, dv, ws)
        return dq, dk, dv, None, None, None


def _attention_lengths(who, lengths, B, T, dev):
    """The frame counts as a device int32 vector, or None.  A host list is checked against [0, T] and uploaded; a device tensor is
    not read here: the kernels clamp it."""
    if lengths is None:
        return None
    if torch.is_tensor(lengths) and lengths.device.type != "cpu":
        if lengths.device != dev:
            raise ValueError("%s: q is on %s and lengths on %s" % (who, dev, lengths.device))
        if lengths.dim() != 1 or lengths.numel() != B or lengths.is_floating_point():
            raise ValueError("%s: expected %d integer lengths, got shape %s %s" % (who, B, tuple(lengths.shape), lengths.dtype))
        return lengths.detach().to(torch.int32).contiguous()
    ln = _lengths(lengths, B, None, who + ": ")
    for b in range(B):
        if not 0 <= ln[b] <= T:
            raise ValueError("%s: utterance %d: %d frames do not lie in [0, %d]" % (who, b, ln[b], T))
    return torch.tensor(ln, dtype=torch.int32).to(dev)


def self_attention(q, k, v, lengths=None, scale=None):
    """``o`` (B, T, H, D) float32 = softmax(scale q k^T) v per utterance and head.  ``q``, ``k``, ``v`` are float32 device tensors
    (B, T, H, D), or (T, H, D) for a batch of one (the result is then (1, T, H, D)); D in {32, 64, 96, 128}, 1 <= H <= 16,
    T <= 4096, B H <= 65 535.  ``lengths`` holds the frames T_b of every utterance, 0 <= T_b <= T: None for T, a host list (checked,
    uploaded) or a device integer tensor (clamped on the device; the call then makes no device-to-host copy, forward or backward).
    ``scale`` defaults to D ** -0.5.  Keys at and beyond T_b do not exist; o is exactly +0 at and beyond T_b, and so are the three
    gradients; NaN in the padding of any operand changes nothing.

    Tensors with unit stride along D whose other strides are multiples of 4 floats and whose storage starts on 16 bytes are read
    as they are, so the three chunks of one packed (B, T, 3 H D) projection cost no copy; anything else is made contiguous.
    Differentiable once with respect to q, k and v; the gradients come back contiguous; a gradient with expanded strides is
    copied.  Under ``no_grad``, or where no input requires a gradient, nothing is kept and the logsumexp is not written;
    otherwise q, k, v, o and a (B, H, T) logsumexp are kept."""
    who = "self_attention"
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise TypeError("%s: expected float32 %s, got %s" % (who, name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if q.dim() == 3 and k.dim() == 3 and v.dim() == 3:
        q, k, v = q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0)
    if q.dim() != 4 or min(q.shape) < 1 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError("%s: expected q, k and v of one shape (B, T, H, D) or (T, H, D), got %s, %s and %s"
                         % (who, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    B, T, H, D = q.shape
    if D % 32 or not MIN_HEAD_WIDTH <= D <= MAX_HEAD_WIDTH:
        raise ValueError("%s: a head width of %d is not one of 32, 64, 96, 128" % (who, D))
    if H > MAX_HEADS:
        raise ValueError("%s: %d heads exceed the limit of %d" % (who, H, MAX_HEADS))
    if T > MAX_FRAMES:
        raise ValueError("%s: %d frames exceed the limit of %d" % (who, T, MAX_FRAMES))
    if B * H > MAX_BATCH_HEADS:
        raise ValueError("%s: %d utterances times %d heads exceed the limit of %d" % (who, B, H, MAX_BATCH_HEADS))
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not 0.0 < float(scale) < float("inf"):
        raise ValueError("%s: the scale must be a positive number, got %r" % (who, scale))
    for name, t in (("k", k), ("v", v)):
        if t.device != q.device:
            raise ValueError("%s: q is on %s and %s on %s" % (who, q.device, name, t.device))
    if not q.is_cuda and not nv.validate_only():
        raise nv.NativeError("%s: q, k and v are on %s; move them to the MI355X first, there is no CPU path" % (who, q.device))
    len_dev = _attention_lengths(who, lengths, B, T, q.device)
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v))
    return _SelfAttention.apply(q, k, v, len_dev, float(scale), keep)


class MultiHeadSelfAttention(torch.nn.Module):
    """The self-attention sublayer of a feed-forward Transformer block: (pre-norm) -> ``qkv_net`` -> ``self_attention`` on the
    three chunks of its output, read as q | k | v along the last axis with the heads contiguous inside each -> ``o_net`` ->
    residual -> (post-norm).  The projections and the norm are torch ops; the attention between them is the native kernel pair,
    which reads the chunks of the packed projection without a copy.

    ``forward(x, lengths)`` takes x (B, T, d_model) and the frames of every utterance as ``self_attention`` does.  The attention
    output is +0 at and beyond T_b, so the rows of the result there are whatever the residual path gives: x itself (and its
    norm after a post-norm), not zeros.  Mask them outside where that matters.  There is no dropout."""

    def __init__(self, n_head, d_model, d_head, pre_lnorm=False):
        super().__init__()
        for name, val in (("n_head", n_head), ("d_model", d_model), ("d_head", d_head)):
            if isinstance(val, bool) or not isinstance(val, int) or val < 1:
                raise ValueError("MultiHeadSelfAttention: %s must be a positive int, got %r" % (name, val))
        if n_head > MAX_HEADS:
            raise ValueError("MultiHeadSelfAttention: %d heads exceed the limit of %d" % (n_head, MAX_HEADS))
        if d_head % 32 or not MIN_HEAD_WIDTH <= d_head <= MAX_HEAD_WIDTH:
            raise ValueError("MultiHeadSelfAttention: a head width of %d is not one of 32, 64, 96, 128" % d_head)
        self.n_head, self.d_model, self.d_head, self.pre_lnorm = n_head, d_model, d_head, bool(pre_lnorm)
        self.scale = 1.0 / math.sqrt(d_head)
        self.qkv_net = torch.nn.Linear(d_model, 3 * n_head * d_head)
        self.o_net = torch.nn.Linear(n_head * d_head, d_model, bias=False)
        self.layer_norm = torch.nn.LayerNorm(d_model)

    def forward(self, x, lengths=None):
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[2] != self.d_model:
            raise ValueError("MultiHeadSelfAttention: expected x (B, T, %d), got %s"
                             % (self.d_model, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        B, T, _ = x.shape
        H, D = self.n_head, self.d_head
        residual = x
        if self.pre_lnorm:
            x = self.layer_norm(x)
        q, k, v = (c.view(B, T, H, D) for c in self.qkv_net(x).chunk(3, dim=2))
        o = self_attention(q, k, v, lengths, self.scale)
        out = residual + self.o_net(o.view(B, T, H * D))
        return out if self.pre_lnorm else self.layer_norm(out)
