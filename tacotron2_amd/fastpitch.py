"""A FastPitch acoustic model on the GPU over the parts of DESIGN.md sections 18 to 23 (csrc/predictor_rows.hip, DESIGN.md section
24): text to mel through a feed-forward Transformer encoder, duration and pitch (and energy) predictors, the length regulator and a
feed-forward Transformer decoder, over a ragged batch.

    y = channel_project(h, weight, bias=None, lengths=None)                 # (B, T, P): h (B, T, C) under weight (P, C), P <= 4
    y = scalar_embed(v, weight, bias=None, lengths=None, base=None)         # (B, T, C): tracks v under weight (C, P, k), + base
    TemporalPredictor(input_size, filter_size, kernel_size, n_layers=2, n_predictions=1)(x, lengths)
    model = FastPitch(n_symbols)
    mel, t_lengths, log_dur, pitch_pred, energy_pred = model(text, durations, pitch)        # teacher-forced
    mel, t_lengths, durations, pitch = model.infer(text, pace=1.0)                          # free-running
    total, parts = FastPitchLoss()(outputs, mel_target, durations, pitch)

The two thin ops are the ends of a temporal predictor the ragged convolution cannot express (it takes multiples of 32 channels on
both sides): native row kernels, one wave per row, exact f32, every sum in a fixed order, no atomics.  As everywhere in this family
an utterance in a ragged batch gives the bits it gives alone, nothing at and beyond T_b is read (NaN there changes nothing) and
every output is exactly +0 there.  There is no CPU path and no dropout."""
import torch

from . import native as nv
from . import ragged as rg
from .alignment import length_regulate
from .transformer import FFTransformer, add_layer_norm, ragged_conv1d

MAX_FRAMES = 4096
MAX_CHANNELS = 4096
MIN_CHANNELS = 32
MAX_KERNEL = 9
MAX_TRACKS = 4
MAX_BATCH = 65535
MAX_MODEL_WIDTH = 512                   # the length regulator's channel limit


def _dense(x):
    """``x`` contiguous float32 on 16 bytes."""
    return rg.aligned(x.float(), strided=False)


def _workspace(dev, *geometry):
    """The workspace ``native.predictor_workspace`` asks for, of 16 bytes at least."""
    return rg.workspace(nv.predictor_workspace(*geometry), dev, least=16)


class _ChannelProject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, weight, bias, len_dev, keep):
        B, T, C = h.shape
        P = weight.shape[0]
        hd, wd = _dense(h.detach()), _dense(weight.detach())
        y = torch.empty(B, T, P, dtype=torch.float32, device=h.device)
        nv.pred_project(hd, wd, None if bias is None else bias.detach().contiguous(), len_dev, y)
        if keep:
            ctx.has_len, ctx.has_bias = len_dev is not None, bias is not None
            ctx.save_for_backward(hd, wd, *(() if len_dev is None else (len_dev,)))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        h, w = ctx.saved_tensors[:2]
        len_dev = ctx.saved_tensors[2] if ctx.has_len else None
        B, T, C = h.shape
        P = w.shape[0]
        dev = h.device
        g = grad.float().contiguous()
        dh = dw = db = None
        if ctx.needs_input_grad[0]:
            dh = torch.empty(B, T, C, dtype=torch.float32, device=dev)
            nv.pred_project_backward(g, w, len_dev, dh)
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:
            dw = torch.empty(P, C, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
            db = torch.empty(P, dtype=torch.float32, device=dev) if want_db else None
            nv.pred_project_sums(g, h, len_dev, dw, db, _workspace(dev, B, T, C, P, 1, 1))
        return dh, dw, db, None, None


class _ScalarEmbed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, weight, bias, base, len_dev, keep):
        B, T, P = v.shape
        C, _, k = weight.shape
        vd = v.detach().float().contiguous()
        image = _dense(weight.detach().permute(1, 2, 0).reshape(P * k, C))  # [p k + j][c]: a torch permute, once a call
        y = torch.empty(B, T, C, dtype=torch.float32, device=v.device)
        nv.pred_embed(vd, image, None if bias is None else _dense(bias.detach()), None if base is None else _dense(base.detach()),
                      len_dev, k, y)
        if keep:
            ctx.has_len, ctx.has_bias, ctx.has_base, ctx.k = len_dev is not None, bias is not None, base is not None, k
            ctx.save_for_backward(vd, image, *(() if len_dev is None else (len_dev,)))
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        v, image = ctx.saved_tensors[:2]
        len_dev = ctx.saved_tensors[2] if ctx.has_len else None
        B, T, P = v.shape
        C, k = image.shape[1], ctx.k
        dev = v.device
        g = _dense(grad)
        want_dv, want_dbase = ctx.needs_input_grad[0], ctx.has_base and ctx.needs_input_grad[3]
        dv = dw = db = dbase = None
        if want_dv or want_dbase:
            dv = torch.empty(B, T, P, dtype=torch.float32, device=dev) if want_dv else None
            dbase = torch.empty(B, T, C, dtype=torch.float32, device=dev) if want_dbase else None
            nv.pred_embed_backward(g, image, len_dev, P, k, dbase, dv)
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:
            dw = torch.empty(C, P, k, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
            db = torch.empty(C, dtype=torch.float32, device=dev) if want_db else None
            nv.pred_embed_sums(g, v, len_dev, k, dw, db, _workspace(dev, B, T, C, P, k, 2))
        return dv, dw, db, dbase, None, None


def _check_batch(who, x):
    if x.shape[1] > MAX_FRAMES:
        raise ValueError("%s: %d frames exceed the limit of %d" % (who, x.shape[1], MAX_FRAMES))
    if x.shape[0] > MAX_BATCH:
        raise ValueError("%s: %d utterances exceed the limit of %d" % (who, x.shape[0], MAX_BATCH))


def _check_channels(who, C):
    if C % 4 or not MIN_CHANNELS <= C <= MAX_CHANNELS:
        raise ValueError("%s: %d channels are not a multiple of 4 from %d to %d" % (who, C, MIN_CHANNELS, MAX_CHANNELS))


def _check_param(who, p, name, shape, dev, owner):
    rg.float32(who, p, name)
    if tuple(p.shape) != tuple(shape):
        raise ValueError("%s: expected %s %s, got %s" % (who, name, tuple(shape), tuple(p.shape)))
    if p.device != dev:
        raise ValueError("%s: %s is on %s and %s on %s" % (who, owner, dev, name, p.device))


def channel_project(h, weight, bias=None, lengths=None):
    """``y`` (B, T, P) float32 = the projection of ``h`` (B, T, C) onto P values per row under ``weight`` (P, C) as ``nn.Linear``
    holds it and ``bias`` (P) or None: for t < T_b, y(b, t, p) = bias(p) + sum_c w(p, c) h(b, t, c); exactly +0 at and beyond
    T_b, where h is never read.  1 <= P <= 4; C a multiple of 4 from 32 to 4096; T <= 4096.  ``lengths`` as ``ragged_conv1d``
    takes them: None for T, a host list (checked, uploaded) or a device integer tensor (clamped on the device; no device-to-host
    copy, forward or backward).

    One wave per row: lane l of 64 chains fmaf over the float4 chunks l, l + 64, .. from +0, the lanes are added by the xor
    butterfly 32 .. 1, then the bias.  Differentiable once: dh = g w (an fmaf chain over p), dw and dbias as sums over the real
    rows in a fixed order.  h and the weight are kept; under ``no_grad`` nothing is."""
    who = "channel_project"
    rg.float32(who, h, "h")
    if h.dim() != 3 or min(h.shape) < 1:
        raise ValueError("%s: expected h (B, T, C), got %s" % (who, tuple(h.shape)))
    _check_batch(who, h)
    B, T, C = h.shape
    _check_channels(who, C)
    rg.float32(who, weight, "weight")
    if weight.dim() != 2 or weight.shape[1] != C:
        raise ValueError("%s: expected weight (P, %d), got %s" % (who, C, tuple(weight.shape)))
    P = weight.shape[0]
    if not 1 <= P <= MAX_TRACKS:
        raise ValueError("%s: %d values per row do not lie in [1, %d]" % (who, P, MAX_TRACKS))
    if weight.device != h.device:
        raise ValueError("%s: h is on %s and weight on %s" % (who, h.device, weight.device))
    if bias is not None:
        _check_param(who, bias, "bias", (P,), h.device, "h")
    rg.require_device(h, who, "h is")
    len_dev = rg.device_lengths(who, lengths, B, T, h.device, "h is")
    keep = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (h, weight, bias))
    return _ChannelProject.apply(h, weight, bias, len_dev, keep)


def scalar_embed(v, weight, bias=None, lengths=None, base=None):
    """``y`` (B, T, C) float32 = the k-tap embedding of the scalar tracks ``v`` (B, T) or (B, T, P) under ``weight`` (C, P, k) as
    ``nn.Conv1d`` holds it, ``bias`` (C) or None, added to ``base`` (B, T, C) or None, with **each utterance embedded as if it were
    alone**: for t < T_b, y(b, t, c) = base(b, t, c) + (bias(c) + sum_{p, j} w(c, p, j) v(b, t + j - k // 2, p)) over the frames
    inside [0, T_b) only; exactly +0 at and beyond T_b, where nothing is read.  1 <= P <= 4; k odd, at most 9; C a multiple of 4
    from 32 to 4096; T <= 4096; ``lengths`` as ``channel_project`` takes them.

    The tap sum is an fmaf chain from +0 over p then j ascending, then the bias, then the base.  The weight image [p k + j][c] is
    a torch permute, made once per call.  Differentiable once: dbase is the gradient masked to the real rows, dv sums the k
    projections of the gradient rows that reach a frame, dw and dbias are sums over the real rows in a fixed order.  v and the
    image are kept; under ``no_grad`` nothing is."""
    who = "scalar_embed"
    rg.float32(who, v, "v")
    if v.dim() == 2:
        v = v.unsqueeze(2)
    if v.dim() != 3 or min(v.shape) < 1:
        raise ValueError("%s: expected v (B, T) or (B, T, P), got %s" % (who, tuple(v.shape)))
    _check_batch(who, v)
    B, T, P = v.shape
    if P > MAX_TRACKS:
        raise ValueError("%s: %d scalar tracks exceed the limit of %d" % (who, P, MAX_TRACKS))
    rg.float32(who, weight, "weight")
    if weight.dim() != 3 or weight.shape[1] != P:
        raise ValueError("%s: expected weight (C, %d, k), got %s" % (who, P, tuple(weight.shape)))
    C, _, k = weight.shape
    if k % 2 == 0 or not 1 <= k <= MAX_KERNEL:
        raise ValueError("%s: a kernel width of %d is not odd and at most %d" % (who, k, MAX_KERNEL))
    _check_channels(who, C)
    if weight.device != v.device:
        raise ValueError("%s: v is on %s and weight on %s" % (who, v.device, weight.device))
    if bias is not None:
        _check_param(who, bias, "bias", (C,), v.device, "v")
    if base is not None:
        _check_param(who, base, "base", (B, T, C), v.device, "v")
    rg.require_device(v, who, "v is")
    len_dev = rg.device_lengths(who, lengths, B, T, v.device, "v is")
    keep = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (v, weight, bias, base))
    return _ScalarEmbed.apply(v, weight, bias, base, len_dev, keep)


def _positive_int(who, name, val, low=1):
    if isinstance(val, bool) or not isinstance(val, int) or val < low:
        raise ValueError("%s: %s must be an int of at least %d, got %r" % (who, name, low, val))


def _odd_kernel(who, name, val):
    if isinstance(val, bool) or not isinstance(val, int) or val % 2 == 0 or not 1 <= val <= MAX_KERNEL:
        raise ValueError("%s: %s must be an odd int up to %d, got %r" % (who, name, MAX_KERNEL, val))


class _ConvNorm(torch.nn.Module):
    """The parameter holders of one predictor layer."""

    def __init__(self, c_in, c_out, k):
        super().__init__()
        self.conv = torch.nn.Conv1d(c_in, c_out, k, padding=k // 2)
        self.norm = torch.nn.LayerNorm(c_out)


class TemporalPredictor(torch.nn.Module):
    """A predictor of ``n_predictions`` values per token: ``n_layers`` of (``ragged_conv1d`` with ReLU, then LayerNorm by
    ``add_layer_norm``), then ``fc`` through ``channel_project``.  ``layers.{i}.conv`` (``nn.Conv1d``), ``layers.{i}.norm``
    (``nn.LayerNorm``) and ``fc`` (``nn.Linear``) only hold the parameters, so the state dict is the ordinary one.
    ``input_size`` and ``filter_size`` are multiples of 32, at most 4096; ``kernel_size`` is odd, at most 9; 1 to 4 predictions.

    ``forward(x, lengths)`` takes x (B, T, input_size) and returns (B, T) for one prediction, else (B, T, n_predictions), +0 at
    and beyond T_b; every utterance is convolved alone.  There is no dropout."""

    def __init__(self, input_size, filter_size, kernel_size, n_layers=2, n_predictions=1):
        super().__init__()
        who = "TemporalPredictor"
        for name, val in (("input_size", input_size), ("filter_size", filter_size)):
            if isinstance(val, bool) or not isinstance(val, int) or val % 32 or not 32 <= val <= MAX_CHANNELS:
                raise ValueError("%s: %s must be a multiple of 32, at most %d, got %r" % (who, name, MAX_CHANNELS, val))
        _odd_kernel(who, "kernel_size", kernel_size)
        _positive_int(who, "n_layers", n_layers)
        _positive_int(who, "n_predictions", n_predictions)
        if n_predictions > MAX_TRACKS:
            raise ValueError("%s: %d predictions exceed the limit of %d" % (who, n_predictions, MAX_TRACKS))
        self.input_size, self.n_predictions = input_size, n_predictions
        self.layers = torch.nn.ModuleList(_ConvNorm(input_size if i == 0 else filter_size, filter_size, kernel_size)
                                          for i in range(n_layers))
        self.fc = torch.nn.Linear(filter_size, n_predictions)

    def forward(self, x, lengths=None):
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[2] != self.input_size:
            raise ValueError("TemporalPredictor: expected x (B, T, %d), got %s"
                             % (self.input_size, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        if lengths is not None:
            lengths = rg.device_lengths("TemporalPredictor", lengths, x.shape[0], x.shape[1], x.device, "x is")
        h = x
        for layer in self.layers:
            h = ragged_conv1d(h, layer.conv.weight, layer.conv.bias, lengths, relu=True)
            h = add_layer_norm(h, None, layer.norm.weight, layer.norm.bias, lengths, layer.norm.eps)
        y = channel_project(h, self.fc.weight, self.fc.bias, lengths)
        return y.squeeze(2) if self.n_predictions == 1 else y


class FastPitch(torch.nn.Module):
    """FastPitch: ``encoder`` (an ``FFTransformer`` behind an embedding of ``n_symbols``), ``duration_predictor`` and
    ``pitch_predictor`` (``TemporalPredictor``s on the encoder output), ``pitch_emb`` (an ``nn.Conv1d(1, d_model, pitch_kernel)``
    holding the parameters of a ``scalar_embed`` that adds the embedded pitch to the encoder output), with ``energy_conditioning``
    the same pair ``energy_predictor`` / ``energy_emb``, the length regulator, ``decoder`` (an ``FFTransformer``) and ``proj``
    (``nn.Linear(d_model, n_mel)``, a torch op, masked by the add-and-mask form of ``add_layer_norm``).  d_model is a multiple of 32,
    at most 512 (the length regulator's limit); n_mel a multiple of 4 from 32.

    ``forward`` is teacher-forced, ``infer`` free-running; both are described there.  There is no dropout, no speaker embedding
    and no learned aligner: durations and token-rate pitch come from outside (``python -m tacotron2_amd.align --token-features``)."""

    def __init__(self, n_symbols, n_mel=80, d_model=384, n_layer=6, n_head=1, d_head=64, d_inner=1536, kernel_size=3,
                 predictor_filter=256, predictor_kernel=3, predictor_layers=2, pitch_kernel=3, energy_conditioning=False,
                 padding_idx=0):
        super().__init__()
        who = "FastPitch"
        _positive_int(who, "n_symbols", n_symbols, 2)
        if isinstance(n_mel, bool) or not isinstance(n_mel, int) or n_mel % 4 or not MIN_CHANNELS <= n_mel <= MAX_CHANNELS:
            raise ValueError("%s: n_mel must be a multiple of 4 from %d to %d, got %r" % (who, MIN_CHANNELS, MAX_CHANNELS, n_mel))
        if isinstance(d_model, bool) or not isinstance(d_model, int) or d_model % 32 or not 32 <= d_model <= MAX_MODEL_WIDTH:
            raise ValueError("%s: d_model must be a multiple of 32, at most %d, got %r" % (who, MAX_MODEL_WIDTH, d_model))
        _odd_kernel(who, "pitch_kernel", pitch_kernel)
        if isinstance(padding_idx, bool) or not isinstance(padding_idx, int) or not 0 <= padding_idx < n_symbols:
            raise ValueError("%s: padding_idx must be an int in [0, %d), got %r" % (who, n_symbols, padding_idx))
        self.n_mel, self.d_model, self.energy_conditioning = n_mel, d_model, bool(energy_conditioning)
        self.encoder = FFTransformer(n_layer, n_head, d_model, d_head, d_inner, kernel_size, n_embed=n_symbols, padding_idx=padding_idx)
        self.decoder = FFTransformer(n_layer, n_head, d_model, d_head, d_inner, kernel_size)
        self.duration_predictor = TemporalPredictor(d_model, predictor_filter, predictor_kernel, predictor_layers)
        self.pitch_predictor = TemporalPredictor(d_model, predictor_filter, predictor_kernel, predictor_layers)
        self.pitch_emb = torch.nn.Conv1d(1, d_model, pitch_kernel, padding=pitch_kernel // 2)
        if self.energy_conditioning:
            self.energy_predictor = TemporalPredictor(d_model, predictor_filter, predictor_kernel, predictor_layers)
            self.energy_emb = torch.nn.Conv1d(1, d_model, pitch_kernel, padding=pitch_kernel // 2)
        self.proj = torch.nn.Linear(d_model, n_mel)

    def _encode(self, text, text_lengths):
        """-> the encoder output (B, N, d_model), the token counts as the device int32 vector every later op takes, and the
        predictions (log durations, pitch, energy or None), each (B, N)."""
        enc, n_dev = self.encoder(text, text_lengths)
        log_dur = self.duration_predictor(enc, n_dev)
        pitch_pred = self.pitch_predictor(enc, n_dev)
        energy_pred = self.energy_predictor(enc, n_dev) if self.energy_conditioning else None
        return enc, n_dev, log_dur, pitch_pred, energy_pred

    def _track(self, who, name, v, text):
        rg.float32(who, v, name)
        if tuple(v.shape) != tuple(text.shape):
            raise ValueError("%s: expected %s of shape %s, got %s" % (who, name, tuple(text.shape), tuple(v.shape)))
        return v

    def _decode(self, who, enc, n_dev, durations, pitch, energy, max_frames):
        h = scalar_embed(pitch, self.pitch_emb.weight, self.pitch_emb.bias, n_dev, base=enc)
        if self.energy_conditioning:
            h = scalar_embed(energy, self.energy_emb.weight, self.energy_emb.bias, n_dev, base=h)
        frames, t_lengths = length_regulate(h, durations, n_dev, T=max_frames)
        if frames.shape[1] < 1:
            raise ValueError("%s: the durations give no frame" % who)
        if frames.shape[1] > MAX_FRAMES:
            raise ValueError("%s: %d frames exceed the limit of %d; name max_frames to cut them" % (who, frames.shape[1], MAX_FRAMES))
        dec, _ = self.decoder(frames, t_lengths)
        return add_layer_norm(self.proj(dec), None, None, None, t_lengths), t_lengths

    def forward(self, text, durations, pitch, energy=None, text_lengths=None, max_frames=None):
        """Teacher-forced: ``text`` (B, N) integer symbols, ``durations`` (B, N) int32 or int64 frames per token, ``pitch`` (and
        with energy conditioning ``energy``) (B, N) float32 at the token rate, ``text_lengths`` as ``FFTransformer`` takes them
        (None counts the symbols that are not ``padding_idx``, on the device).  The predictors read the encoder output; the
        targets, not the predictions, are embedded and regulated.  -> (mel (B, T, n_mel), t_lengths (B,) int32, log_dur_pred
        (B, N), pitch_pred (B, N), energy_pred (B, N) or None), each exactly +0 beyond its lengths.  T is ``max_frames``, or
        with None the batch's longest sum of durations, found by the length regulator's one device-to-host read; with
        ``max_frames`` an int and device lengths the call never synchronises."""
        who = "FastPitch"
        if not torch.is_tensor(text) or text.dim() != 2 or text.is_floating_point():
            raise ValueError("%s: expected integer symbols (B, N), got %s"
                             % (who, tuple(text.shape) if torch.is_tensor(text) else type(text).__name__))
        pitch = self._track(who, "pitch", pitch, text)
        if self.energy_conditioning:
            if energy is None:
                raise ValueError("%s: energy conditioning needs the energy targets" % who)
            energy = self._track(who, "energy", energy, text)
        elif energy is not None:
            raise ValueError("%s: energy targets were given to a model without energy conditioning" % who)
        enc, n_dev, log_dur, pitch_pred, energy_pred = self._encode(text, text_lengths)
        mel, t_lengths = self._decode(who, enc, n_dev, durations, pitch, energy, max_frames)
        return mel, t_lengths, log_dur, pitch_pred, energy_pred

    @torch.no_grad()
    def infer(self, text, text_lengths=None, pace=1.0, pitch_transform=None, max_frames=None, max_duration=75):
        """Free-running, under ``no_grad``: durations = clamp(round((exp(log_dur_pred) - 1) / pace), 0, ``max_duration``) on the
        device (the rounding rule of ``LengthRegulator``), the predicted pitch (and energy) in place of the targets, the pitch
        first passed through ``pitch_transform(pitch, lengths)`` where given, then the path of ``forward``.  -> (mel, t_lengths,
        durations (B, N) int32, pitch (B, N)): the mel ``forward`` gives for these durations and this pitch (and the predicted
        energy), bit for bit."""
        who = "FastPitch.infer"
        pace = rg.positive(who, pace, "the pace must be a positive number")
        _positive_int(who, "max_duration", max_duration, 0)
        enc, n_dev, log_dur, pitch, energy = self._encode(text, text_lengths)
        durations = torch.round((torch.exp(log_dur) - 1.0) / pace).clamp_(0, max_duration).to(torch.int32)
        if pitch_transform is not None:
            pitch = pitch_transform(pitch, n_dev)
            self._track(who, "the transformed pitch", pitch, text)
        mel, t_lengths = self._decode(who, enc, n_dev, durations, pitch, energy, max_frames)
        return mel, t_lengths, durations, pitch


class FastPitchLoss(torch.nn.Module):
    """The training loss of ``FastPitch.forward``, in torch ops: the mean squared error of the mel over the real frames, plus
    ``dur_scale`` times that of ``log_dur_pred`` against log(1 + durations) over the real tokens, plus ``pitch_scale`` (and
    ``energy_scale``) times that of the pitch (and energy) prediction against the target over the real tokens.

    ``forward(outputs, mel, durations, pitch, energy=None, text_lengths=None)`` takes the tuple ``FastPitch.forward`` returned,
    the target mel (B, T', n_mel) with T' at least the output's T, and the targets the model was fed; ``text_lengths`` is a device
    integer tensor or None for all N tokens.  What lies beyond a length is never used (NaN there changes nothing).  -> (total,
    dict of the unscaled parts), all device scalars; nothing is copied to the host."""

    def __init__(self, dur_scale=0.1, pitch_scale=0.1, energy_scale=0.1):
        super().__init__()
        for name, val in (("dur_scale", dur_scale), ("pitch_scale", pitch_scale), ("energy_scale", energy_scale)):
            if isinstance(val, bool) or not isinstance(val, (int, float)) or not 0.0 <= float(val) < float("inf"):
                raise ValueError("FastPitchLoss: %s must be a finite number that is not negative, got %r" % (name, val))
        self.dur_scale, self.pitch_scale, self.energy_scale = float(dur_scale), float(pitch_scale), float(energy_scale)

    @staticmethod
    def _masked_mse(pred, target, live, count):
        diff = torch.where(live, pred - target, pred.new_zeros(()))
        return (diff * diff).sum() / count

    def forward(self, outputs, mel, durations, pitch, energy=None, text_lengths=None):
        mel_out, t_lengths, log_dur, pitch_pred, energy_pred = outputs
        B, T, n_mel = mel_out.shape
        N = log_dur.shape[1]
        if mel.dim() != 3 or mel.shape[0] != B or mel.shape[1] < T or mel.shape[2] != n_mel:
            raise ValueError("FastPitchLoss: expected a target mel (%d, at least %d, %d), got %s" % (B, T, n_mel, tuple(mel.shape)))
        if (energy is None) != (energy_pred is None):
            raise ValueError("FastPitchLoss: energy targets and an energy prediction are given together or not at all")
        dev = mel_out.device
        frames = t_lengths.clamp(0, T)
        live_t = torch.arange(T, device=dev)[None, :] < frames[:, None]
        n_frames = frames.sum().clamp(min=1).to(torch.float32)
        parts = dict(mel=self._masked_mse(mel_out, mel[:, :T], live_t[:, :, None], n_frames * n_mel))
        if text_lengths is None:
            live_n = torch.ones(B, N, dtype=torch.bool, device=dev)
            n_tokens = float(B * N)
        else:
            tokens = text_lengths.to(dev).clamp(0, N)
            live_n = torch.arange(N, device=dev)[None, :] < tokens[:, None]
            n_tokens = tokens.sum().clamp(min=1).to(torch.float32)
        parts["duration"] = self._masked_mse(log_dur, torch.log1p(durations.to(log_dur.dtype).clamp(min=0)), live_n, n_tokens)
        parts["pitch"] = self._masked_mse(pitch_pred, pitch, live_n, n_tokens)
        total = parts["mel"] + self.dur_scale * parts["duration"] + self.pitch_scale * parts["pitch"]
        if energy is not None:
            parts["energy"] = self._masked_mse(energy_pred, energy, live_n, n_tokens)
            total = total + self.energy_scale * parts["energy"]
        return total, parts
