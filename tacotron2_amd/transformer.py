"""Masked multi-head self-attention on the GPU (csrc/self_attn.hip, csrc/self_attn_rows.hip): the middle of
the feed-forward Transformer block of FastSpeech, FastPitch and FastSpeech 2, over a ragged batch.

    o = self_attention(q, k, v, lengths=None, scale=None)                   # (B, T, H, D), differentiable once
    y = MultiHeadSelfAttention(n_head, d_model, d_head, pre_lnorm=False)(x, lengths)

Per utterance b with T_b = lengths[b] frames and per head: p(t, .) = softmax over j < T_b of scale q(t, .) . k(j, .), o(t, :) =
sum_j p(t, j) v(j, :) for t < T_b and exactly +0 from there on.  A fused kernel pair on the exact-f32 matrix pipe: the forward
keeps a running maximum and sum per row, the backward recomputes the probabilities from the kept logsumexp, so no (T, T) matrix
exists in memory.  Exact f32 products, every sum in a fixed ascending order, no atomics: two calls give the same bits, and an
utterance in a ragged batch gives the bits it gives alone.  What lies at and beyond T_b in q, k, v and the gradient is never
read.  There is no CPU path.

The other half of the block (csrc/fft_block.hip, csrc/fft_block_rows.hip):

    y = ragged_conv1d(x, weight, bias, lengths, relu=False)                 # (B, T, Cout): each utterance convolved alone
    y = add_layer_norm(x, residual, weight, bias, lengths, eps=1e-5)        # LayerNorm(x + residual), +0 at and beyond T_b
    PositionwiseConvFF(d_model, d_inner, kernel_size), FFTBlock(n_head, d_model, d_head, d_inner, kernel_size),
    FFTransformer(n_layer, n_head, d_model, d_head, d_inner, kernel_size, n_embed=None)"""
import math

import torch

from . import native as nv
from . import ragged as rg

MAX_FRAMES = 4096
MAX_HEADS = 16
MIN_HEAD_WIDTH = 32
MAX_HEAD_WIDTH = 128
MAX_BATCH_HEADS = 65535


class _SelfAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, len_dev, scale, keep):
        B, T, H, D = q.shape
        dev = q.device
        qd, kd, vd = (rg.aligned(t.detach()) for t in (q, k, v))     # the chunks of a packed projection pass as they are
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
        g = rg.aligned(grad.float())
        dq, dk, dv = (torch.empty(B, T, H, D, dtype=torch.float32, device=q.device) for _ in range(3))
        ws = rg.workspace(nv.self_attn_workspace(B, T, H, D, 2), q.device)
        nv.self_attn_backward(q, k, v, o, lse, g, len_dev, ctx.scale, dq, dk, dv, ws)
        return dq, dk, dv, None, None, None


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
        rg.float32(who, t, name)
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
    scale = rg.positive(who, scale, "the scale must be a positive number", bools=False)
    for name, t in (("k", k), ("v", v)):
        if t.device != q.device:
            raise ValueError("%s: q is on %s and %s on %s" % (who, q.device, name, t.device))
    rg.require_device(q, who, "q, k and v are")
    len_dev = rg.device_lengths(who, lengths, B, T, q.device, "q is")
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v))
    return _SelfAttention.apply(q, k, v, len_dev, scale, keep)


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


# ---- the convolutional feed-forward and add + LayerNorm (csrc/fft_block.hip, csrc/fft_block_rows.hip) -------------------------------
MAX_CHANNELS = 4096
MAX_KERNEL = 9
MIN_NORM_CHANNELS = 32
MAX_BATCH = 65535


def _dense(x):
    """``x`` contiguous float32 on 16 bytes."""
    return rg.aligned(x.float(), strided=False)


def _workspace(dev, *geometry):
    """The workspace ``native.fft_block_workspace`` asks for, of 16 bytes at least."""
    return rg.workspace(nv.fft_block_workspace(*geometry), dev, least=16)


class _RaggedConv1d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, len_dev, relu, keep):
        B, T, Cin = x.shape
        Cout, _, k = weight.shape
        xd, wd = rg.aligned(x.detach()), weight.detach()
        image = _dense(wd.permute(0, 2, 1).reshape(Cout, k * Cin))          # [o][j Cin + i]: a torch permute, once a call
        y = torch.empty(B, T, Cout, dtype=torch.float32, device=x.device)
        nv.ffb_conv(xd, image, None if bias is None else _dense(bias.detach()), None, len_dev, k, relu, y)
        if keep:
            ctx.relu, ctx.has_len, ctx.has_bias = relu, len_dev is not None, bias is not None
            ctx.save_for_backward(xd, wd, *((y,) if relu else ()), *(() if len_dev is None else (len_dev,)))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        saved = list(ctx.saved_tensors)
        x, w = saved[0], saved[1]
        y = saved[2] if ctx.relu else None
        len_dev = saved[-1] if ctx.has_len else None
        B, T, Cin = x.shape
        Cout, _, k = w.shape
        dev = x.device
        g = _dense(grad)
        if ctx.relu:                                                        # the masked gradient, written once for all three
            gm = torch.empty_like(g)
            nv.ffb_relu_mask(g, y, len_dev, gm)
            g = gm
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            image = _dense(w.flip(2).permute(1, 2, 0).reshape(Cin, k * Cout))   # [i][j Cout + o] = w(o, i, k - 1 - j)
            dx = torch.empty(B, T, Cin, dtype=torch.float32, device=dev)
            nv.ffb_conv(g, image, None, None, len_dev, k, False, dx)
        if ctx.needs_input_grad[1]:
            dw = torch.empty(Cout, Cin, k, dtype=torch.float32, device=dev)
            nv.ffb_conv_dw(g, x, len_dev, k, dw, _workspace(dev, B, T, Cin, Cout, k, 1))
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = torch.empty(Cout, dtype=torch.float32, device=dev)
            nv.ffb_colsum(g, None, None, None, len_dev, db, None, _workspace(dev, B, T, Cout, Cout, 1, 2))
        return dx, dw, db, None, None, None


class _AddLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, len_dev, eps, keep):
        B, T, C = x.shape
        dev = x.device
        xd = _dense(x.detach())
        rd = None if residual is None else _dense(residual.detach())
        y = torch.empty(B, T, C, dtype=torch.float32, device=dev)
        norm = weight is not None
        z = mean = rstd = None
        if keep and norm:
            z = torch.empty(B, T, C, dtype=torch.float32, device=dev)
            mean, rstd = (torch.empty(B, T, dtype=torch.float32, device=dev) for _ in range(2))
        wd = _dense(weight.detach()) if norm else None
        nv.ffb_add_ln(xd, rd, wd, _dense(bias.detach()) if norm else None, len_dev, eps, y, z, mean, rstd)
        if keep:
            ctx.norm, ctx.has_len, ctx.has_res, ctx.eps = norm, len_dev is not None, residual is not None, eps
            ctx.save_for_backward(*((z, mean, rstd, wd) if norm else ()), *(() if len_dev is None else (len_dev,)))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        saved = list(ctx.saved_tensors)
        len_dev = saved[-1] if ctx.has_len else None
        g = _dense(grad)
        dz = torch.empty_like(g)
        dw = db = None
        if not ctx.norm:
            nv.ffb_add_ln(g, None, None, None, len_dev, ctx.eps, dz)        # the masked gradient
        else:
            z, mean, rstd, w = saved[:4]
            B, T, C = z.shape
            nv.ffb_add_ln_backward(g, z, mean, rstd, w, len_dev, dz)
            if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
                dw, db = (torch.empty(C, dtype=torch.float32, device=g.device) for _ in range(2))
                nv.ffb_colsum(g, z, mean, rstd, len_dev, db, dw, _workspace(g.device, B, T, C, C, 1, 2))
        return dz, (dz if ctx.has_res else None), dw, db, None, None, None


def _check_rows(who, x, name="x"):
    rg.float32(who, x, name)
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError("%s: expected %s (B, T, C), got %s" % (who, name, tuple(x.shape)))
    if x.shape[1] > MAX_FRAMES:
        raise ValueError("%s: %d frames exceed the limit of %d" % (who, x.shape[1], MAX_FRAMES))
    if x.shape[0] > MAX_BATCH:
        raise ValueError("%s: %d utterances exceed the limit of %d" % (who, x.shape[0], MAX_BATCH))


def _check_param(who, p, name, shape, dev):
    rg.float32(who, p, name)
    if tuple(p.shape) != tuple(shape):
        raise ValueError("%s: expected %s %s, got %s" % (who, name, tuple(shape), tuple(p.shape)))
    if p.device != dev:
        raise ValueError("%s: x is on %s and %s on %s" % (who, dev, name, p.device))


def ragged_conv1d(x, weight, bias=None, lengths=None, relu=False):
    """``y`` (B, T, Cout) float32 = the convolution over time of ``x`` (B, T, Cin) under ``weight`` (Cout, Cin, k) as ``nn.Conv1d``
    holds it and ``bias`` (Cout) or None, with **each utterance convolved as if it were alone**: for t < T_b,
    y(b, t, o) = act(bias(o) + sum_{j, i} w(o, i, j) x(b, t + j - k // 2, i)) over the frames inside [0, T_b) only; act is the
    identity or, with ``relu``, max(., 0).  y is exactly +0 at and beyond T_b, rows of x there are never read (NaN planted there
    changes nothing), and so it is for the gradient.  ``lengths`` as ``self_attention`` takes them: None for T, a host list
    (checked, uploaded) or a device integer tensor (clamped on the device; no device-to-host copy, forward or backward).

    k is odd, at most 9; Cin and Cout are multiples of 32, at most 4096; T <= 4096.  x is read as it is where its channel stride
    is 1, its other strides are multiples of 4 floats and its storage starts on 16 bytes; anything else is copied.  Exact f32
    products on the matrix pipe, the sum over (tap, channel) ascending then the bias.  The two weight images (tap-major, and
    flipped and transposed for dx) are torch permutes, made once per call.  Differentiable once: dx, dw (sum over b, then t
    ascending) and dbias; with ``relu`` the gradient is first multiplied by [y > 0].  x, the weight and, with ``relu``, y are kept;
    under ``no_grad`` nothing is."""
    who = "ragged_conv1d"
    _check_rows(who, x)
    rg.float32(who, weight, "weight")
    B, T, Cin = x.shape
    if weight.dim() != 3 or weight.shape[1] != Cin:
        raise ValueError("%s: expected weight (Cout, %d, k), got %s" % (who, Cin, tuple(weight.shape)))
    Cout, _, k = weight.shape
    if k % 2 == 0 or not 1 <= k <= MAX_KERNEL:
        raise ValueError("%s: a kernel width of %d is not odd and at most %d" % (who, k, MAX_KERNEL))
    for name, c in (("input", Cin), ("output", Cout)):
        if c % 32 or not 32 <= c <= MAX_CHANNELS:
            raise ValueError("%s: %d %s channels are not a multiple of 32, at most %d" % (who, c, name, MAX_CHANNELS))
    if weight.device != x.device:
        raise ValueError("%s: x is on %s and weight on %s" % (who, x.device, weight.device))
    if bias is not None:
        _check_param(who, bias, "bias", (Cout,), x.device)
    rg.require_device(x, who, "x is")
    len_dev = rg.device_lengths(who, lengths, B, T, x.device, "x is")
    keep = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias))
    return _RaggedConv1d.apply(x, weight, bias, len_dev, bool(relu), keep)


def add_layer_norm(x, residual=None, weight=None, bias=None, lengths=None, eps=1e-5):
    """``y`` (B, T, C) float32 = LayerNorm(x + residual) weight + bias over C for every row t < T_b (mean and a two-pass variance in
    one wave per row), exactly +0 at and beyond T_b, where nothing is read.  ``residual`` may be None.  ``weight`` and ``bias``
    both None: "add and mask only", y = x + residual below T_b and +0 beyond.  C is a multiple of 4, 32 <= C <= 4096; ``lengths``
    as ``ragged_conv1d`` takes them.  Differentiable once: the LayerNorm input gradient is returned for both x and residual,
    dweight and dbias are column sums over the real rows in a fixed order.  z = x + residual and the (B, T) mean and rstd are
    kept (only the lengths without a weight); under ``no_grad`` nothing is."""
    who = "add_layer_norm"
    _check_rows(who, x)
    B, T, C = x.shape
    if C % 4 or not MIN_NORM_CHANNELS <= C <= MAX_CHANNELS:
        raise ValueError("%s: %d channels are not a multiple of 4 from %d to %d" % (who, C, MIN_NORM_CHANNELS, MAX_CHANNELS))
    if residual is not None:
        _check_param(who, residual, "residual", x.shape, x.device)
    if (weight is None) != (bias is None):
        raise ValueError("%s: weight and bias are given together or not at all" % who)
    if weight is not None:
        _check_param(who, weight, "weight", (C,), x.device)
        _check_param(who, bias, "bias", (C,), x.device)
    eps = rg.positive(who, eps, "eps must be a positive number", bools=False)
    rg.require_device(x, who, "x is")
    len_dev = rg.device_lengths(who, lengths, B, T, x.device, "x is")
    keep = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, residual, weight, bias))
    return _AddLayerNorm.apply(x, residual, weight, bias, len_dev, eps, keep)


class PositionwiseConvFF(torch.nn.Module):
    """The convolutional feed-forward sublayer of a feed-forward Transformer block: (pre-norm) -> conv1 + ReLU -> conv2 ->
    residual add + LayerNorm (post-norm), or the plain masked add after a pre-norm.  ``conv1``, ``conv2`` (``nn.Conv1d``) and
    ``layer_norm`` only hold the parameters, so the state dict is the ordinary one; the work is ``ragged_conv1d`` and
    ``add_layer_norm``.  ``kernel_size`` is an int or a pair (FastSpeech 2 uses (9, 1)).

    ``forward(x, lengths)`` takes x (B, T, d_model).  Each utterance is convolved alone, the input's rows at and beyond T_b are
    never read and the result is +0 there, so no mask is needed around it.  There is no dropout."""

    def __init__(self, d_model, d_inner, kernel_size, pre_lnorm=False):
        super().__init__()
        ks = tuple(kernel_size) if isinstance(kernel_size, (tuple, list)) else (kernel_size, kernel_size)
        if len(ks) != 2 or any(isinstance(k, bool) or not isinstance(k, int) or k % 2 == 0 or not 1 <= k <= MAX_KERNEL for k in ks):
            raise ValueError("PositionwiseConvFF: kernel_size must be an odd int up to %d or a pair of them, got %r" % (MAX_KERNEL, kernel_size))
        for name, val in (("d_model", d_model), ("d_inner", d_inner)):
            if isinstance(val, bool) or not isinstance(val, int) or val % 32 or not 32 <= val <= MAX_CHANNELS:
                raise ValueError("PositionwiseConvFF: %s must be a multiple of 32, at most %d, got %r" % (name, MAX_CHANNELS, val))
        self.d_model, self.d_inner, self.kernel_size, self.pre_lnorm = d_model, d_inner, ks, bool(pre_lnorm)
        self.conv1 = torch.nn.Conv1d(d_model, d_inner, ks[0], padding=ks[0] // 2)
        self.conv2 = torch.nn.Conv1d(d_inner, d_model, ks[1], padding=ks[1] // 2)
        self.layer_norm = torch.nn.LayerNorm(d_model)

    def forward(self, x, lengths=None):
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[2] != self.d_model:
            raise ValueError("PositionwiseConvFF: expected x (B, T, %d), got %s"
                             % (self.d_model, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        ln = self.layer_norm
        if lengths is not None:
            lengths = rg.device_lengths("PositionwiseConvFF", lengths, x.shape[0], x.shape[1], x.device, "x is")
        h = add_layer_norm(x, None, ln.weight, ln.bias, lengths, ln.eps) if self.pre_lnorm else x
        h = ragged_conv1d(h, self.conv1.weight, self.conv1.bias, lengths, relu=True)
        h = ragged_conv1d(h, self.conv2.weight, self.conv2.bias, lengths)
        if self.pre_lnorm:
            return add_layer_norm(h, x, None, None, lengths)
        return add_layer_norm(h, x, ln.weight, ln.bias, lengths, ln.eps)


class FFTBlock(torch.nn.Module):
    """One feed-forward Transformer block: ``MultiHeadSelfAttention`` then ``PositionwiseConvFF``, both over the same lengths.
    The result is +0 at and beyond T_b.  There is no dropout."""

    def __init__(self, n_head, d_model, d_head, d_inner, kernel_size, pre_lnorm=False):
        super().__init__()
        self.dec_attn = MultiHeadSelfAttention(n_head, d_model, d_head, pre_lnorm=pre_lnorm)
        self.pos_ff = PositionwiseConvFF(d_model, d_inner, kernel_size, pre_lnorm=pre_lnorm)

    def forward(self, x, lengths=None):
        if lengths is not None and torch.is_tensor(x) and x.dim() == 3:
            lengths = rg.device_lengths("FFTBlock", lengths, x.shape[0], x.shape[1], x.device, "x is")
        return self.pos_ff(self.dec_attn(x, lengths), lengths)


def positional_embedding(T, d_model, lengths=None, device=None):
    """(1 or B, T, d_model) float32: [sin(t f_i) | cos(t f_i)] with f_i = 10000 ** (-2 i / d_model), i < d_model / 2; with device
    ``lengths`` (B,) the rows at and beyond T_b are zero."""
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0.0, d_model, 2.0, device=device) / d_model))
    pos = torch.arange(T, device=device, dtype=torch.float32)
    ang = pos[:, None] * inv_freq[None, :]
    emb = torch.cat([ang.sin(), ang.cos()], dim=1)[None]
    if lengths is None:
        return emb
    live = torch.arange(T, device=device)[None, :] < lengths[:, None]
    return torch.where(live[:, :, None], emb, emb.new_zeros(()))            # +0, where a product would leave -0


class FFTransformer(torch.nn.Module):
    """A stack of ``n_layer`` ``FFTBlock``s behind an optional ``nn.Embedding`` (``n_embed`` symbols, ``padding_idx``) and the
    sinusoidal positional embedding, which is computed per call, is zero at and beyond T_b and is added before the first block.
    ``forward(x, lengths)`` takes x (B, T, d_model) float32, or (B, T) integer symbols with an embedding (``lengths`` None then
    counts the symbols that are not ``padding_idx``, on the device), and returns (out, lengths) with out +0 at and beyond T_b and
    the lengths as the device int32 vector the blocks used (None for full length).  There is no dropout."""

    def __init__(self, n_layer, n_head, d_model, d_head, d_inner, kernel_size, pre_lnorm=False, n_embed=None, padding_idx=0):
        super().__init__()
        if isinstance(n_layer, bool) or not isinstance(n_layer, int) or n_layer < 1:
            raise ValueError("FFTransformer: n_layer must be a positive int, got %r" % (n_layer,))
        self.d_model, self.padding_idx = d_model, padding_idx
        self.word_emb = None if n_embed is None else torch.nn.Embedding(n_embed, d_model, padding_idx=padding_idx)
        self.layers = torch.nn.ModuleList(FFTBlock(n_head, d_model, d_head, d_inner, kernel_size, pre_lnorm=pre_lnorm)
                                          for _ in range(n_layer))

    def forward(self, x, lengths=None):
        if self.word_emb is not None:
            if not torch.is_tensor(x) or x.dim() != 2 or x.is_floating_point():
                raise ValueError("FFTransformer: expected integer symbols (B, T), got %s"
                                 % ((tuple(x.shape) if torch.is_tensor(x) else type(x).__name__),))
            if lengths is None:
                lengths = (x != self.padding_idx).sum(dim=1)
            x = self.word_emb(x)
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[2] != self.d_model:
            raise ValueError("FFTransformer: expected x (B, T, %d), got %s"
                             % (self.d_model, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        B, T, _ = x.shape
        len_dev = rg.device_lengths("FFTransformer", lengths, B, T, x.device, "x is")
        out = x + positional_embedding(T, self.d_model, None if len_dev is None else len_dev.clamp(0, T), x.device)
        for layer in self.layers:
            out = layer(out, len_dev)
        return out, len_dev
