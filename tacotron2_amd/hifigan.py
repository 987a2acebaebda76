"""HiFi-GAN generator (Kong, Kim, Bae 2020) on the MI355X: mel -> waveform, inference only.

    hg = load_hifigan("generator_v1").cuda().eval()    # {'generator': state dict}, weight_g / weight_v or folded
    audio = hg(mel)                                     # (B, 80, N) log-mels -> (B, 1, 256 N) float32 in (-1, 1)
    audio = hg.infer(mel, lengths=frames)               # ragged: every utterance as if alone, zero beyond 256 n_b

The module keeps the published submodule names (``conv_pre``, ``ups.{i}``, ``resblocks.{i n_k + j}.convs1.{m}`` /
``.convs2.{m}`` or ``.convs.{m}``, ``conv_post``), so ``state_dict()`` keys are those of a checkpoint after
``remove_weight_norm``; a weight-normed checkpoint is folded on load (``fold_weight_norm``).  The geometry is read from the
tensor shapes; dilations and upsample rates are not in the shapes: dilations default to the published values per resblock
type and kernel list, rates to half the transposed kernels (every published stage).  Weights are f32 masters;
``precision`` selects the compute of the products as in ``WaveGlow``: 'fp32' (exact f32 MFMA), 'bf16x3' or 'bf16'.
``.half()`` keeps the f32 weights, selects 'bf16' and returns float16.

Per call: one mel-packing launch, conv_pre, per stage one transposed-convolution launch (all phases) and one launch per
resblock convolution (t2amd_hg_conv_f32: the leaky-ReLU on the operand, the residual and the multi-receptive-field sum in
the epilogue), conv_post with tanh.  One workspace allocation per call; the stage loop does no allocation, copy or host
synchronisation and has no loop over utterances.  Channel counts below 32 (V2's last stages) run zero-padded to 32.
Training the generator and its discriminators is out of scope; the mel-reconstruction term of its objective exists on its
own (``tacotron2_amd.audio.MelLoss``), but the generator has no backward pass to feed it into.  The arithmetic is restated in float64 torch by
tests/hifigan_ref.py; DESIGN.md section 11 has the layout.
"""
import numpy as np
import torch
from torch import nn

from . import native as nv
from .vocoder import PRECISIONS, Vocoder, checkpoint_source, packed_rows
from .waveglow import fold_weight_norm

LRELU_SLOPE = 0.1
POST_SLOPE = 0.01                 # the reference's last leaky_relu is called without a slope: torch's default
PRE_KERNEL = POST_KERNEL = 7
MAX_ROWS = 2 ** 31 - 256          # the rows of the widest stage (csrc/common.h T2_MAX_ROWS)
MAX_CHANNELS = 512
MAX_POST_CHANNELS = 64


def default_dilations(resblock, kernel_sizes):
    """The published dilations: (1, 3, 5) for every type '1' block; (1, 2), (2, 6), (3, 12) for the type '2' kernels 3, 5, 7
    (any other type '2' kernel list gets (1, 3) for each, the block's own default)."""
    if resblock == '1':
        return [(1, 3, 5) for _ in kernel_sizes]
    if tuple(kernel_sizes) == (3, 5, 7):
        return [(1, 2), (2, 6), (3, 12)]
    return [(1, 3) for _ in kernel_sizes]


def config_from_state_dict(state_dict, upsample_rates=None, resblock_dilation_sizes=None):
    """Generator constructor arguments from the tensor shapes of a (folded or weight-normed) generator state dict."""
    sd = state_dict

    def w(name):
        for suffix in ('.weight', '.weight_v'):
            if name + suffix in sd:
                return sd[name + suffix]
        raise KeyError("HiFi-GAN: missing %s.weight" % name)

    ups = sorted({int(k.split('.')[1]) for k in sd if k.startswith('ups.')})
    blocks = sorted({int(k.split('.')[1]) for k in sd if k.startswith('resblocks.')})
    if not ups or ups != list(range(len(ups))) or not blocks or blocks != list(range(len(blocks))) or len(blocks) % len(ups):
        raise ValueError("HiFi-GAN: no ups.<i> / resblocks.<j> layers of a generator in the state dict")
    n_k = len(blocks) // len(ups)
    resblock = '1' if any(k.startswith('resblocks.0.convs1.') for k in sd) else '2'
    sub = 'convs1' if resblock == '1' else 'convs'
    ks = [int(w('resblocks.%d.%s.0' % (j, sub)).shape[2]) for j in range(n_k)]
    n_dil = [len({k.split('.')[3] for k in sd if k.startswith('resblocks.%d.%s.' % (j, sub))}) for j in range(n_k)]
    dil = list(resblock_dilation_sizes) if resblock_dilation_sizes is not None else default_dilations(resblock, ks)
    if [len(d) for d in dil] != n_dil:
        raise ValueError("HiFi-GAN: the state dict has %s convolutions per resblock, the dilations %s" % (n_dil, dil))
    uks = [int(w('ups.%d' % i).shape[2]) for i in ups]
    rates = list(upsample_rates) if upsample_rates is not None else [k // 2 for k in uks]
    pre = w('conv_pre')
    return dict(n_mel_channels=int(pre.shape[1]), upsample_initial_channel=int(pre.shape[0]), upsample_rates=rates,
                upsample_kernel_sizes=uks, resblock=resblock, resblock_kernel_sizes=ks, resblock_dilation_sizes=dil)


class ResBlock1(nn.Module):
    def __init__(self, channels, kernel_size, dilation):
        super().__init__()
        self.convs1 = nn.ModuleList([nn.Conv1d(channels, channels, kernel_size, dilation=d, padding=d * (kernel_size - 1) // 2)
                                     for d in dilation])
        self.convs2 = nn.ModuleList([nn.Conv1d(channels, channels, kernel_size, padding=(kernel_size - 1) // 2)
                                     for _ in dilation])


class ResBlock2(nn.Module):
    def __init__(self, channels, kernel_size, dilation):
        super().__init__()
        self.convs = nn.ModuleList([nn.Conv1d(channels, channels, kernel_size, dilation=d, padding=d * (kernel_size - 1) // 2)
                                    for d in dilation])


def _ce(c):
    """Channels as the kernels see them: a multiple of 32, at least 32 (the padding carries zero weights and biases)."""
    return max(32, -(-c // 32) * 32)


def pack_conv(weight, bias, ci_e, co_e):
    """Conv1d weight [Co][Ci][k] -> [Co_e][k * Ci_e] (K tap-major: column tap * Ci_e + c), bias -> [Co_e]; zero padding."""
    w = weight.float()
    co, ci, k = w.shape
    wp = torch.zeros(co_e, k, ci_e, dtype=torch.float32, device=w.device)
    wp[:co, :, :ci] = w.permute(0, 2, 1)
    b = torch.zeros(co_e, dtype=torch.float32, device=w.device)
    b[:co] = bias.float()
    return wp.reshape(co_e, k * ci_e), b


def pack_up(weight, bias, u, ci_e, co_e):
    """ConvTranspose1d weight [Ci][Co][ku] -> [u][Co_e][(ku / u) * Ci_e]: phase p, q = p + (ku - u) / 2, takes the taps
    kk = q % u + u j, which read input row m + q // u - j; bias -> [Co_e]; zero padding."""
    w = weight.float()
    ci, co, ku = w.shape
    pad, taps = (ku - u) // 2, ku // u
    wp = torch.zeros(u, co_e, taps, ci_e, dtype=torch.float32, device=w.device)
    for p in range(u):
        for j in range(taps):
            wp[p, :co, j, :ci] = w[:, :, (p + pad) % u + u * j].t()
    b = torch.zeros(co_e, dtype=torch.float32, device=w.device)
    b[:co] = bias.float()
    return wp.reshape(u, co_e, taps * ci_e), b


class Generator(Vocoder):
    LABEL = 'HiFi-GAN'

    def __init__(self, n_mel_channels=80, upsample_initial_channel=512, upsample_rates=(8, 8, 2, 2),
                 upsample_kernel_sizes=(16, 16, 4, 4), resblock='1', resblock_kernel_sizes=(3, 7, 11),
                 resblock_dilation_sizes=None, precision='fp32'):
        super().__init__()
        resblock = str(resblock)
        rates, uks, ks = list(upsample_rates), list(upsample_kernel_sizes), list(resblock_kernel_sizes)
        dil = [tuple(d) for d in (resblock_dilation_sizes if resblock_dilation_sizes is not None
                                  else default_dilations(resblock, ks))]
        C0 = int(upsample_initial_channel)
        if resblock not in ('1', '2'):
            raise ValueError("HiFi-GAN: resblock must be '1' or '2', got %r" % resblock)
        if not rates or len(rates) != len(uks) or not ks or len(dil) != len(ks) or any(len(d) < 1 for d in dil):
            raise ValueError("HiFi-GAN: %d upsample rates for %d kernels, %d resblock kernels for %d dilation lists"
                             % (len(rates), len(uks), len(ks), len(dil)))
        for k in ks:
            if k < 1 or k % 2 == 0:
                raise ValueError("HiFi-GAN: resblock kernel %d is even; the padding d (k - 1) / 2 keeps the length for odd "
                                 "kernels only" % k)
        if any(d < 1 for dd in dil for d in dd):
            raise ValueError("HiFi-GAN: dilations must be positive, got %s" % (dil,))
        for u, ku in zip(rates, uks):
            if u < 1 or u > 64 or ku < u:
                raise ValueError("HiFi-GAN: upsample rate %d with kernel %d (rates 1 to 64, kernel >= rate)" % (u, ku))
            if (ku - u) % 2:
                raise ValueError("HiFi-GAN: upsample kernel %d - rate %d is odd; padding (ku - u) / 2 gives u times the "
                                 "rows for an even difference only" % (ku, u))
            if ku % u:
                raise ValueError("HiFi-GAN: upsample kernel %d is not a multiple of the rate %d (the polyphase product "
                                 "needs ku / u taps per phase)" % (ku, u))
        if C0 % (2 ** len(rates)) or C0 < 2 ** len(rates):
            raise ValueError("HiFi-GAN: %d initial channels cannot be halved %d times" % (C0, len(rates)))
        chans = [C0 // 2 ** i for i in range(len(rates) + 1)]
        for c in chans:
            if _ce(c) > MAX_CHANNELS or (c > 32 and c % 32):
                raise ValueError("HiFi-GAN: %d channels are not covered by the kernels (a multiple of 32 up to %d, or fewer "
                                 "than 32)" % (c, MAX_CHANNELS))
        if _ce(chans[-1]) > MAX_POST_CHANNELS:
            raise ValueError("HiFi-GAN: conv_post takes at most %d channels, this geometry ends with %d"
                             % (MAX_POST_CHANNELS, chans[-1]))
        if n_mel_channels < 1 or _ce(n_mel_channels) > MAX_CHANNELS:
            raise ValueError("HiFi-GAN: n_mel_channels must be 1 to %d, got %d" % (MAX_CHANNELS, n_mel_channels))
        self.n_mel_channels, self.upsample_initial_channel = int(n_mel_channels), C0
        self.upsample_rates, self.upsample_kernel_sizes = rates, uks
        self.resblock, self.resblock_kernel_sizes, self.resblock_dilation_sizes = resblock, ks, dil
        self.channels = chans
        self.num_kernels, self.num_upsamples = len(ks), len(rates)
        self.hop = int(np.prod(rates))
        self.conv_pre = nn.Conv1d(n_mel_channels, C0, PRE_KERNEL, padding=PRE_KERNEL // 2)
        self.ups = nn.ModuleList([nn.ConvTranspose1d(chans[i], chans[i + 1], ku, stride=u, padding=(ku - u) // 2)
                                  for i, (u, ku) in enumerate(zip(rates, uks))])
        block = ResBlock1 if resblock == '1' else ResBlock2
        self.resblocks = nn.ModuleList([block(chans[i + 1], k, d) for i in range(len(rates)) for k, d in zip(ks, dil)])
        self.conv_post = nn.Conv1d(chans[-1], 1, POST_KERNEL, padding=POST_KERNEL // 2)
        self.precision = precision

    def config(self):
        return dict(n_mel_channels=self.n_mel_channels, upsample_initial_channel=self.upsample_initial_channel,
                    upsample_rates=list(self.upsample_rates), upsample_kernel_sizes=list(self.upsample_kernel_sizes),
                    resblock=self.resblock, resblock_kernel_sizes=list(self.resblock_kernel_sizes),
                    resblock_dilation_sizes=[tuple(d) for d in self.resblock_dilation_sizes])

    def remove_weight_norm(self):
        """The reference's call before inference: the module is always folded, so there is nothing to remove."""
        return self

    # ---- loading ------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Takes a folded state dict or a weight-normed one (``weight_g`` / ``weight_v``, folded here)."""
        sd = fold_weight_norm(dict(state_dict))
        try:
            cfg = config_from_state_dict(sd, upsample_rates=self.upsample_rates,
                                         resblock_dilation_sizes=self.resblock_dilation_sizes)
        except ValueError as e:
            raise ValueError("HiFi-GAN: state dict geometry does not match the module's %s: %s" % (self.config(), e))
        if cfg != self.config():
            raise ValueError("HiFi-GAN: state dict geometry %s does not match the module's %s" % (cfg, self.config()))
        self._pack = None
        return super().load_state_dict(self._f32_state(sd), strict=strict, assign=assign)

    @classmethod
    def from_state_dict(cls, state_dict, precision='fp32', upsample_rates=None, resblock_dilation_sizes=None):
        sd = fold_weight_norm(dict(state_dict))
        m = cls(precision=precision, **config_from_state_dict(sd, upsample_rates, resblock_dilation_sizes))
        m.load_state_dict(sd)
        return m

    # ---- row plan -----------------------------------------------------------------------------------------------------
    def stage_scales(self):
        """Rows per mel frame of stage 0 (conv_pre's output) .. n_up (the waveform rate)."""
        return [int(np.prod(self.upsample_rates[:i])) for i in range(self.num_upsamples + 1)]

    def row_windows(self):
        """[(stage of the rows read, lowest row offset, highest row offset)] of every launch: the operand rows a launch
        reads for output row r of the same space (for a transposed convolution: for the rows of input row r)."""
        out = [(0, -(PRE_KERNEL // 2), PRE_KERNEL // 2)]
        for i, (u, ku) in enumerate(zip(self.upsample_rates, self.upsample_kernel_sizes)):
            pad, taps = (ku - u) // 2, ku // u
            out.append((i, 0 - (taps - 1), (u - 1 + pad) // u))
            for k, dil in zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes):
                for d in dil:
                    out.append((i + 1, -d * (k - 1) // 2, d * (k - 1) // 2))
                    if self.resblock == '1':
                        out.append((i + 1, -(k - 1) // 2, (k - 1) // 2))
        out.append((self.num_upsamples, -(POST_KERNEL // 2), POST_KERNEL // 2))
        return out

    def halo_frames(self):
        """H0: zero frame-level rows before, between and after the utterances, so that H0 * (rows per frame of a stage)
        covers the widest window of that stage."""
        sc = self.stage_scales()
        return max(-(-max(-lo, hi) // sc[s]) for s, lo, hi in self.row_windows())

    def packed_plan(self, lengths):
        """(rowb0, rowr0, offsets, P0) of the frame-level packed row space for per-utterance frame counts (host tensors)."""
        return packed_rows(lengths, self.halo_frames())

    def workspace_floats(self, P0):
        """Floats of the one allocation of a call with P0 frame-level packed rows: four stage images of the widest stage and
        the packed mels."""
        sc = self.stage_scales()
        widest = max(P0 * s * _ce(c) for s, c in zip(sc, self.channels))
        return 4 * widest + P0 * _ce(self.n_mel_channels), widest

    def _plan(self, lens, dev):
        def build():
            rowb0, rowr0, offs, P0 = self.packed_plan(lens)
            if P0 * self.hop > MAX_ROWS:
                raise ValueError("HiFi-GAN: %d packed frames x %d samples per frame exceed the %d rows one call can address; "
                                 "split the batch" % (P0, self.hop, MAX_ROWS))
            return rowb0.to(dev), rowr0.to(dev), P0
        return self._cached_plan((tuple(lens), str(dev)), build)

    # ---- device-side weight layout ------------------------------------------------------------------------------------
    def _packed(self, device):
        key = self._pack_key(device)
        if self._pack is not None and self._pack[0] == key:
            return self._pack[1]

        def conv(m, ci_e, co_e):
            return pack_conv(m.weight.detach().to(device), m.bias.detach().to(device), ci_e, co_e)

        def up(m, u, ci_e, co_e):
            return pack_up(m.weight.detach().to(device), m.bias.detach().to(device), u, ci_e, co_e)

        with torch.no_grad():
            ce = [_ce(c) for c in self.channels]
            pk = dict(pre=conv(self.conv_pre, _ce(self.n_mel_channels), ce[0]), ups=[], blocks=[])
            for i, u in enumerate(self.upsample_rates):
                pk['ups'].append(up(self.ups[i], u, ce[i], ce[i + 1]))
                for j in range(self.num_kernels):
                    blk = self.resblocks[i * self.num_kernels + j]
                    c = ce[i + 1]
                    if self.resblock == '1':
                        pk['blocks'].append([(conv(a, c, c), conv(b, c, c)) for a, b in zip(blk.convs1, blk.convs2)])
                    else:
                        pk['blocks'].append([(conv(a, c, c), None) for a in blk.convs])
            pw = self.conv_post.weight.detach().float()
            post = torch.zeros(POST_KERNEL, ce[-1], dtype=torch.float32, device=device)
            post[:, :pw.shape[1]] = pw[0].t()
            pk['post'] = (post, self.conv_post.bias.detach().float().contiguous())
        self._pack = (key, pk)
        return pk

    # ---- inference ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def infer(self, mel, lengths=None):
        """(B, n_mel, N) log-mels (float32 / float16 / bfloat16) -> (B, 1, hop N) audio (float16 after ``.half()``).
        ``lengths``: frames per utterance (ragged: each computed as if alone, zero beyond hop n_b)."""
        dev = self._device()
        B, nm, N, lens = self._check_mels(mel, lengths, "infer")
        prec = PRECISIONS[self.precision]
        rowb0, rowr0, P0 = self._plan(lens, dev)
        total, widest = self.workspace_floats(P0)
        self._check_free(dev, total + B * self.hop * N, total, P0, "infer")
        pk = self._packed(dev)
        x32 = mel.to(device=dev, dtype=torch.float32).contiguous()
        ws = torch.empty(total, dtype=torch.float32, device=dev)
        out = torch.zeros(B, 1, self.hop * N, dtype=torch.float32, device=dev)
        bufs = [ws[i * widest:(i + 1) * widest] for i in range(4)]
        mel_cl = ws[4 * widest:].view(P0, _ce(nm))

        def img(k, rows, c):
            return bufs[k][:rows * c].view(rows, c)

        ce = [_ce(c) for c in self.channels]
        inv = float(np.float32(1.0) / np.float32(self.num_kernels))
        # buffers: 0 the stage's input x, 1 / 2 the resblock's running x and its inner activation, 3 the fusion sum
        nv.hg_pack_mel(x32, rowb0, rowr0, mel_cl)
        nv.hg_conv(mel_cl, pk['pre'][0], pk['pre'][1], PRE_KERNEL, 1, None, None, img(3, P0, ce[0]), 1.0, False, rowb0, 1, prec)
        scale = 1
        for i, (u, ku) in enumerate(zip(self.upsample_rates, self.upsample_kernel_sizes)):
            P, c = P0 * scale * u, ce[i + 1]
            x = img(0, P, c)
            nv.hg_upsample(img(3, P0 * scale, ce[i]), pk['ups'][i][0], pk['ups'][i][1], ku, u, LRELU_SLOPE, x, rowb0, scale, prec)
            scale *= u
            s = img(3, P, c)
            for j, k in enumerate(self.resblock_kernel_sizes):
                layers = pk['blocks'][i * self.num_kernels + j]
                dil = self.resblock_dilation_sizes[j]
                cur, cur_k = x, 0
                for m, ((w1, b1), second) in enumerate(layers):
                    last = m == len(layers) - 1
                    if second is not None:
                        t = img(2, P, c)
                        nv.hg_conv(cur, w1, b1, k, dil[m], LRELU_SLOPE, None, t, 1.0, False, rowb0, scale, prec)
                        src, w, b, d = t, second[0], second[1], 1
                    else:
                        src, w, b, d = cur, w1, b1, dil[m]
                    if last:
                        nv.hg_conv(src, w, b, k, d, LRELU_SLOPE, cur, s, inv, j > 0, rowb0, scale, prec)
                    else:
                        # type '1' updates the running x in place (its product reads t, and every element of the residual is
                        # read and written by the same lane); type '2' reads the rows it adds to, so it alternates buffers
                        dst_k = 1 if second is not None or cur_k != 1 else 2
                        dst = img(dst_k, P, c)
                        nv.hg_conv(src, w, b, k, d, LRELU_SLOPE, cur, dst, 1.0, False, rowb0, scale, prec)
                        cur, cur_k = dst, dst_k
        nv.hg_post(img(3, P0 * scale, ce[-1]), pk['post'][0], pk['post'][1], POST_SLOPE, rowb0, rowr0, scale, out)
        return self._io(out)

    def forward(self, mel):
        """The reference's ``forward`` is its inference."""
        return self.infer(mel)


def load_hifigan(src, precision='fp32'):
    """A Generator from a checkpoint path, a state dict, ``{'generator': state dict or module}`` or a module."""
    return Generator._from_source(checkpoint_source(src, 'generator'), "load_hifigan", precision=precision)
