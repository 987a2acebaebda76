"""Vocos vocoder (Siuzdak 2023) on the MI355X: mel -> waveform at the frame rate, inference and a backward pass.

    vc = load_vocos("vocos_mel_22khz.pt").cuda().eval()   # a state dict, {'state_dict': ...} or a module
    audio = vc(mel)                                         # (B, 80, N) log-mels -> (B, 1, 256 N) float32
    audio = vc.infer(mel, lengths=frames)                   # ragged: every utterance as if alone, zero beyond hop n_b
    audio = vc.generate(mel); loss(audio).backward()        # infer's bits with a grad_fn: gradients of every parameter (and mel)
    MelLoss(stft)(vc.generate(mel), mel).backward()         # the mel-reconstruction loss (tacotron2_amd.audio); a driver around
                                                            # this step is tacotron2_amd.vocos_train

A ConvNeXt stack on D-channel frame rows, one linear head that predicts log-magnitude and phase, one inverse STFT: nothing
runs at the sample rate before the overlap-add.  The module keeps the published names (``backbone.embed``, ``backbone.norm``,
``backbone.convnext.{i}.dwconv`` / ``.norm`` / ``.pwconv1`` / ``.pwconv2`` / ``.gamma``, ``backbone.final_layer_norm``,
``head.out``, ``head.istft.window``); ``feature_extractor.*`` keys of a published checkpoint are ignored (the mel front end is
this project's), a checkpoint with an ``adanorm`` backbone (EnCodec features) is refused.  The geometry is read from the
tensor shapes; hop and padding are not in the shapes: they default to n_fft / 4 and 'same'.  Weights are f32 masters;
``precision`` selects the compute of the two products of every block: 'fp32' (exact f32 MFMA), 'bf16x3' or 'bf16'.  The head
product and the inverse DFT stay at f32 or split-bf16 even with 'bf16': phase error goes straight into the waveform.
``.half()`` keeps the f32 weights, selects 'bf16' and returns float16.

Per call: mel packing, embed, LayerNorm; per block three launches (dwconv + LayerNorm, pwconv1 + GELU, pwconv2 with gamma and
the residual); LayerNorm, head, polar, inverse DFT, overlap-add.  One workspace allocation per call; the layer loop does no
allocation, copy or host synchronisation and has no loop over utterances.  The arithmetic is restated in float64 torch by
tests/vocos_ref.py; DESIGN.md section 12 has the layout.

``generate`` is ``infer`` as one autograd function: it keeps ``saved_state_bytes(P)`` in one allocation (the mel rows, every
LayerNorm input, every block's normalised rows and GELU output, the head rows) and its backward runs the row kernels of
csrc/vocos_bwd.hip between ``vc_linear`` products against transposed weight images and fixed-order split-K weight-gradient
products; the pre-GELU rows and the pre-gamma ``pwconv2`` output are recomputed, one product each.
"""
import numpy as np
import torch
from torch import nn

from . import native as nv
from .hifigan import _ce, pack_conv
from .vocoder import PRECISIONS, Vocoder, checkpoint_source, packed_rows, _splitk, _wgrad

EMBED_KERNEL = DW_KERNEL = 7
LN_EPS = 1e-6
MAG_CLAMP = 100.0
HALO = 3                          # zero rows around every utterance: the 7-tap windows, and (n_fft - hop) / hop frames of tail
MAX_ROWS = 2 ** 31 - 256          # csrc/common.h T2_MAX_ROWS
MAX_DIM = 512
MAX_INTERMEDIATE = 2048
MAX_N_FFT = 16384
PADDINGS = ('same', 'center')


def _pad_cols(n):
    """Columns of the head product: a multiple of 32, and of 128 (the widest tile) once there is more than one such tile."""
    return -(-n // 32) * 32 if n <= 128 else -(-n // 128) * 128


def config_from_state_dict(state_dict, hop_length=None, padding='same'):
    """Vocos constructor arguments from the tensor shapes of a state dict."""
    sd = state_dict
    bad = sorted(k for k in sd if 'adanorm' in k or k.endswith('.norm.scale.weight') or k.endswith('.norm.shift.weight'))
    if bad:
        raise ValueError("Vocos: the checkpoint has an adanorm backbone (%s ...): EnCodec-feature models are not covered, only "
                         "the mel models with LayerNorm" % bad[0])
    for k in ('backbone.embed.weight', 'backbone.convnext.0.pwconv1.weight', 'head.out.weight'):
        if k not in sd:
            raise ValueError("Vocos: missing %s: not a Vocos state dict" % k)
    layers = sorted({int(k.split('.')[2]) for k in sd if k.startswith('backbone.convnext.')})
    if layers != list(range(len(layers))):
        raise ValueError("Vocos: backbone.convnext layers %s are not 0 .. L-1" % layers)
    emb = sd['backbone.embed.weight']
    two_f = int(sd['head.out.weight'].shape[0])
    n_fft = two_f - 2
    if emb.dim() != 3 or emb.shape[2] != EMBED_KERNEL or two_f < 4 or two_f % 2:
        raise ValueError("Vocos: embed %s / head.out %s are not Conv1d(n_mel, D, 7) and Linear(D, n_fft + 2)"
                         % (tuple(emb.shape), tuple(sd['head.out.weight'].shape)))
    if 'head.istft.window' in sd and sd['head.istft.window'].numel() != n_fft:
        raise ValueError("Vocos: head.istft.window has %d samples, head.out predicts n_fft = %d"
                         % (sd['head.istft.window'].numel(), n_fft))
    return dict(n_mel_channels=int(emb.shape[1]), dim=int(emb.shape[0]),
                intermediate_dim=int(sd['backbone.convnext.0.pwconv1.weight'].shape[0]), num_layers=len(layers), n_fft=n_fft,
                hop_length=int(hop_length) if hop_length is not None else n_fft // 4, padding=padding)


class ConvNeXtBlock(nn.Module):
    def __init__(self, dim, intermediate_dim):
        super().__init__()
        self.dwconv = nn.Conv1d(dim, dim, DW_KERNEL, padding=DW_KERNEL // 2, groups=dim)
        self.norm = nn.LayerNorm(dim, eps=LN_EPS)
        self.pwconv1 = nn.Linear(dim, intermediate_dim)
        self.pwconv2 = nn.Linear(intermediate_dim, dim)
        self.gamma = nn.Parameter(torch.full((dim,), 1.0 / 8))


class Backbone(nn.Module):
    def __init__(self, n_mel_channels, dim, intermediate_dim, num_layers):
        super().__init__()
        self.embed = nn.Conv1d(n_mel_channels, dim, EMBED_KERNEL, padding=EMBED_KERNEL // 2)
        self.norm = nn.LayerNorm(dim, eps=LN_EPS)
        self.convnext = nn.ModuleList([ConvNeXtBlock(dim, intermediate_dim) for _ in range(num_layers)])
        self.final_layer_norm = nn.LayerNorm(dim, eps=LN_EPS)


class ISTFT(nn.Module):
    def __init__(self, n_fft):
        super().__init__()
        self.register_buffer('window', torch.hann_window(n_fft, periodic=True))


class Head(nn.Module):
    def __init__(self, dim, n_fft):
        super().__init__()
        self.out = nn.Linear(dim, n_fft + 2)
        self.istft = ISTFT(n_fft)


def inverse_basis(window):
    """[n_fft][ceil32(n_fft + 2)] float32: frame[t] = sum_k S[2k] basis[t][2k] + S[2k+1] basis[t][2k+1] is
    window[t] irfft(S, n_fft)[t] for interleaved (re, im) rows S; built in float64 with exact angle reduction."""
    w = window.detach().double().cpu()
    L = w.numel()
    F = L // 2 + 1
    t = torch.arange(L, dtype=torch.int64)[:, None]
    k = torch.arange(F, dtype=torch.int64)[None, :]
    ang = ((t * k) % L).double() * (2.0 * np.pi / L)
    c = torch.full((F,), 2.0, dtype=torch.float64)
    c[0] = c[-1] = 1.0
    out = torch.zeros(L, -(-2 * F // 32) * 32, dtype=torch.float64)
    out[:, 0:2 * F:2] = torch.cos(ang) * c * (w[:, None] / L)
    out[:, 1:2 * F:2] = -torch.sin(ang) * c * (w[:, None] / L)
    out[:, 1] = 0.0                       # irfft ignores the imaginary parts of DC and Nyquist
    out[:, 2 * F - 1] = 0.0
    return out.float()


class Vocos(Vocoder):
    LABEL = 'Vocos'

    def __init__(self, n_mel_channels=80, dim=512, intermediate_dim=1536, num_layers=8, n_fft=1024, hop_length=256,
                 padding='same', precision='fp32'):
        super().__init__()
        D, I, L, hop = int(dim), int(intermediate_dim), int(n_fft), int(hop_length)
        if D < 32 or D % 32 or D > MAX_DIM:
            raise ValueError("Vocos: dim %d is not covered by the kernels (a multiple of 32 up to %d)" % (D, MAX_DIM))
        if I < 32 or I % 32 or I > MAX_INTERMEDIATE:
            raise ValueError("Vocos: intermediate_dim %d is not covered by the kernels (a multiple of 32 up to %d)"
                             % (I, MAX_INTERMEDIATE))
        if num_layers < 1:
            raise ValueError("Vocos: num_layers must be at least 1, got %d" % num_layers)
        if n_mel_channels < 1 or _ce(n_mel_channels) > MAX_DIM:
            raise ValueError("Vocos: n_mel_channels must be 1 to %d, got %d" % (MAX_DIM, n_mel_channels))
        if L < 32 or L % 32 or L > MAX_N_FFT:
            raise ValueError("Vocos: n_fft %d is not covered by the kernels (a multiple of 32 up to %d)" % (L, MAX_N_FFT))
        if hop < 1 or L % hop:
            raise ValueError("Vocos: hop %d does not divide n_fft %d (the overlap-added window must be periodic in hop)" % (hop, L))
        if (L - hop) % 2:
            raise ValueError("Vocos: n_fft %d - hop %d is odd; the 'same' trim (n_fft - hop) / 2 is whole for an even "
                             "difference only" % (L, hop))
        if 2 * hop > L or L // hop - 1 > HALO:
            raise ValueError("Vocos: hop %d with n_fft %d: 2 to %d frames must overlap (the %d halo rows hold an utterance's "
                             "tail)" % (hop, L, HALO + 1, HALO))
        if padding not in PADDINGS:
            raise ValueError("Vocos: padding must be 'same' or 'center', got %r" % (padding,))
        self.n_mel_channels, self.dim, self.intermediate_dim, self.num_layers = int(n_mel_channels), D, I, int(num_layers)
        self.n_fft, self.hop, self.padding = L, hop, padding
        self.backbone = Backbone(self.n_mel_channels, D, I, self.num_layers)
        self.head = Head(D, L)
        self.precision = precision
        self._pack_t = None

    hop_length = property(lambda self: self.hop)

    def config(self):
        return dict(n_mel_channels=self.n_mel_channels, dim=self.dim, intermediate_dim=self.intermediate_dim,
                    num_layers=self.num_layers, n_fft=self.n_fft, hop_length=self.hop, padding=self.padding)

    # ---- loading ------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Takes a Vocos state dict; ``feature_extractor.*`` keys (the published mel front end) are dropped."""
        sd = {k: v for k, v in state_dict.items() if not k.startswith('feature_extractor.')}
        cfg = config_from_state_dict(sd, hop_length=self.hop, padding=self.padding)
        if cfg != self.config():
            raise ValueError("Vocos: state dict geometry %s does not match the module's %s" % (cfg, self.config()))
        self._pack = None
        return super().load_state_dict(self._f32_state(sd), strict=strict, assign=assign)

    @classmethod
    def from_state_dict(cls, state_dict, precision='fp32', hop_length=None, padding='same'):
        sd = {k: v for k, v in state_dict.items() if not k.startswith('feature_extractor.')}
        m = cls(precision=precision, **config_from_state_dict(sd, hop_length, padding))
        m.load_state_dict(sd)
        return m

    # ---- row plan -----------------------------------------------------------------------------------------------------
    def trim(self):
        """Samples cut from each end of an utterance's overlap-add."""
        return (self.n_fft - self.hop) // 2 if self.padding == 'same' else self.n_fft // 2

    def samples(self, n):
        """Samples of an utterance of n frames."""
        return self.hop * n if self.padding == 'same' else self.hop * (n - 1)

    def row_windows(self):
        """[(lowest row offset, highest row offset)] of every launch that reads other rows than its own: embed, every dwconv,
        and the overlap-add (the rows whose frames reach the samples of row r's hop, either padding)."""
        reach = self.n_fft // self.hop - 1
        return [(-(EMBED_KERNEL // 2), EMBED_KERNEL // 2)] + [(-(DW_KERNEL // 2), DW_KERNEL // 2)] * self.num_layers + \
            [(-reach, reach)]

    def packed_plan(self, lengths):
        """(rowb0, rowr0, utt, offsets, P) of the packed row space for per-utterance frame counts (host tensors)."""
        rowb, rowr, offs, P = packed_rows(lengths, HALO)
        utt = torch.tensor([[o, int(n)] for o, n in zip(offs, lengths)], dtype=torch.int32)
        return rowb, rowr, utt, offs, P

    def row_widths(self):
        """Floats per packed row of the workspace regions: mels, two D-wide images, the intermediate, head, spectrum, frames."""
        two_f = self.n_fft + 2
        return [_ce(self.n_mel_channels), self.dim, self.dim, self.intermediate_dim, _pad_cols(two_f), -(-two_f // 32) * 32,
                self.n_fft]

    def workspace_floats(self, P):
        return P * sum(self.row_widths())

    def _plan(self, lens, dev):
        def build():
            rowb0, rowr0, utt, offs, P = self.packed_plan(lens)
            if P > MAX_ROWS:
                raise ValueError("Vocos: %d packed frames exceed the %d rows one call can address; split the batch"
                                 % (P, MAX_ROWS))
            return rowb0.to(dev), rowr0.to(dev), utt.to(dev), P
        return self._cached_plan((tuple(lens), str(dev)), build)

    # ---- device-side weight layout ------------------------------------------------------------------------------------
    def _packed(self, device):
        key = self._pack_key(device)
        if self._pack is not None and self._pack[0] == key:
            return self._pack[1]

        def f(t):
            return t.detach().to(device=device, dtype=torch.float32).contiguous()

        with torch.no_grad():
            bb, two_f = self.backbone, self.n_fft + 2
            pk = dict(embed=pack_conv(bb.embed.weight.detach().to(device), bb.embed.bias.detach().to(device),
                                      _ce(self.n_mel_channels), self.dim),
                      norm=(f(bb.norm.weight), f(bb.norm.bias)), final=(f(bb.final_layer_norm.weight), f(bb.final_layer_norm.bias)),
                      blocks=[])
            for blk in bb.convnext:
                pk['blocks'].append(dict(dw=(f(blk.dwconv.weight[:, 0, :].t()), f(blk.dwconv.bias)),
                                         norm=(f(blk.norm.weight), f(blk.norm.bias)),
                                         pw1=(f(blk.pwconv1.weight), f(blk.pwconv1.bias)),
                                         pw2=(f(blk.pwconv2.weight), f(blk.pwconv2.bias)), gamma=f(blk.gamma)))
            nh = _pad_cols(two_f)
            hw = torch.zeros(nh, self.dim, dtype=torch.float32, device=device)
            hb = torch.zeros(nh, dtype=torch.float32, device=device)
            hw[:two_f], hb[:two_f] = f(self.head.out.weight), f(self.head.out.bias)
            pk['head'] = (hw, hb)
            win = self.head.istft.window
            pk['basis'] = inverse_basis(win).to(device)
            pk['wsq'] = (win.detach().double().cpu() ** 2).float().to(device)
        self._pack = (key, pk)
        return pk

    # ---- inference ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def infer(self, mel, lengths=None):
        """(B, n_mel, N) log-mels (float32 / float16 / bfloat16) -> (B, 1, hop N) audio ('center': hop (N - 1); float16 after
        ``.half()``).  ``lengths``: frames per utterance (ragged: each computed as if alone, zero beyond its samples)."""
        dev = self._device()
        B, nm, N, lens = self._check_mels(mel, lengths, "infer")
        T = self.samples(N)
        if T < 1 or B > 65535:
            raise ValueError("Vocos.infer: %d utterances of %d frames give %d samples with padding %r (1 to 65535 utterances, "
                             "at least one sample)" % (B, N, T, self.padding))
        prec = PRECISIONS[self.precision]
        head_prec = min(prec, 1)
        rowb0, rowr0, utt, P = self._plan(lens, dev)
        total = self.workspace_floats(P)
        self._check_free(dev, total + B * T, total, P, "infer")
        pk = self._packed(dev)
        x32 = mel.to(device=dev, dtype=torch.float32).contiguous()
        ws = torch.empty(total, dtype=torch.float32, device=dev)
        out = torch.empty(B, 1, T, dtype=torch.float32, device=dev)
        mel_cl, x, t, h, y, spec, frames = self._regions(ws, P, self.row_widths())
        nv.hg_pack_mel(x32, rowb0, rowr0, mel_cl)
        nv.hg_conv(mel_cl, pk['embed'][0], pk['embed'][1], EMBED_KERNEL, 1, None, None, t, 1.0, False, rowb0, 1, prec)
        nv.vc_dwln(t, None, None, pk['norm'][0], pk['norm'][1], LN_EPS, rowb0, x)
        for blk in pk['blocks']:
            nv.vc_dwln(x, blk['dw'][0], blk['dw'][1], blk['norm'][0], blk['norm'][1], LN_EPS, rowb0, t)
            nv.vc_linear(t, blk['pw1'][0], blk['pw1'][1], 'gelu', None, None, h, rowb0, prec)
            nv.vc_linear(h, blk['pw2'][0], blk['pw2'][1], 'residual', blk['gamma'], x, x, rowb0, prec)
        nv.vc_dwln(x, None, None, pk['final'][0], pk['final'][1], LN_EPS, rowb0, t)
        nv.vc_linear(t, pk['head'][0], pk['head'][1], None, None, None, y, rowb0, head_prec)
        nv.vc_polar(y, self.n_fft // 2 + 1, MAG_CLAMP, rowb0, spec)
        nv.vc_linear(spec, pk['basis'], None, None, None, None, frames, rowb0, head_prec)
        nv.vc_ola(frames, pk['wsq'], utt, self.hop, self.trim(), out)
        return self._io(out)

    def forward(self, mel):
        """The reference's ``decode`` of mel features."""
        return self.infer(mel)

    # ---- training: infer with a backward pass ---------------------------------------------------------------------------
    def saved_row_widths(self):
        """Floats per packed row of what ``generate`` keeps: the mel rows, embed's output, the input of every block and of
        the final LayerNorm (L + 1 images), per block the normalised rows and the GELU output, the final LayerNorm's output
        and the head rows."""
        D, I, L = self.dim, self.intermediate_dim, self.num_layers
        return [_ce(self.n_mel_channels), D] + [D] * (L + 1) + [D] * L + [I] * L + [D, _pad_cols(self.n_fft + 2)]

    def saved_state_bytes(self, P):
        """Bytes ``generate`` keeps between its forward and its backward for P packed rows, in one allocation:
        4 P (ce(n_mel) + (2 L + 3) D + L I + head columns)."""
        return 4 * int(P) * sum(self.saved_row_widths())

    def _fwd_widths(self):
        """The forward's workspace beside the kept state: spectrum and frames."""
        return [-(-(self.n_fft + 2) // 32) * 32, self.n_fft]

    def _check_state(self, need, extra, free, P):
        """Refuse a ``generate`` whose kept state (``need`` bytes) plus ``extra`` bytes of workspace and output do not fit."""
        if need + extra > free:
            raise nv.NativeError("Vocos.generate: the state kept for the backward pass needs %.2f GB (%d packed rows x %d "
                                 "floats) and %.2f GB are free; use a smaller batch or shorter segments"
                                 % (need / 1e9, P, sum(self.saved_row_widths()), free / 1e9))

    def generate(self, mel, lengths=None):
        """``infer`` with a backward pass: the same launches, so the same bits, as a float32 tensor with a ``grad_fn`` when
        gradients are enabled and a parameter or ``mel`` requires grad.  ``backward()`` gives every parameter that requires
        grad its float32 gradient (``head.istft.window`` is a buffer and gets none) and ``mel`` its own, zero beyond each
        utterance's frames.  ``precision`` selects the compute of the backward's products as of the forward's; the head, the
        inverse DFT and their backward stay at f32 or split-bf16.  Training keeps float32 in and out: a ``.half()`` module is
        refused.  ``saved_state_bytes(P)`` are kept in one allocation; a state that does not fit is refused before any launch.
        Under ``torch.no_grad()`` this is ``infer``."""
        if self.half_io:
            raise ValueError("Vocos.generate: the module was set to .half(); training keeps float32 in and out (call .float() "
                             "and choose the compute with precision='bf16')")
        params = list(self.parameters())
        if torch.is_grad_enabled() and (any(p.requires_grad for p in params) or (torch.is_tensor(mel) and mel.requires_grad)):
            return _Generate.apply(self, mel, lengths, *params)
        return self.infer(mel, lengths)

    def _generate_forward(self, mel, lengths):
        """``infer``'s launches with their row images kept -> (audio, kept state)."""
        dev = self._device()
        B, nm, N, lens = self._check_mels(mel, lengths, "generate")
        T = self.samples(N)
        if T < 1 or B > 65535:
            raise ValueError("Vocos.generate: %d utterances of %d frames give %d samples with padding %r (1 to 65535 "
                             "utterances, at least one sample)" % (B, N, T, self.padding))
        prec = PRECISIONS[self.precision]
        head_prec = min(prec, 1)
        rowb0, rowr0, utt, P = self._plan(lens, dev)
        L = self.num_layers
        need, total = self.saved_state_bytes(P), P * sum(self._fwd_widths())
        if dev.type == 'cuda':
            free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
            self._check_state(need, 4 * (total + B * T), free, P)
        pk = self._packed(dev)
        x32 = mel.detach().to(device=dev, dtype=torch.float32).contiguous()
        state = torch.empty(need // 4, dtype=torch.float32, device=dev)
        ws = torch.empty(total, dtype=torch.float32, device=dev)
        out = torch.empty(B, 1, T, dtype=torch.float32, device=dev)
        kept = self._regions(state, P, self.saved_row_widths())
        mel_cl, e, xs, ts, hs, tf, y = kept[0], kept[1], kept[2:L + 3], kept[L + 3:2 * L + 3], kept[2 * L + 3:3 * L + 3], \
            kept[3 * L + 3], kept[3 * L + 4]
        spec, frames = self._regions(ws, P, self._fwd_widths())
        nv.hg_pack_mel(x32, rowb0, rowr0, mel_cl)
        nv.hg_conv(mel_cl, pk['embed'][0], pk['embed'][1], EMBED_KERNEL, 1, None, None, e, 1.0, False, rowb0, 1, prec)
        nv.vc_dwln(e, None, None, pk['norm'][0], pk['norm'][1], LN_EPS, rowb0, xs[0])
        for i, blk in enumerate(pk['blocks']):
            nv.vc_dwln(xs[i], blk['dw'][0], blk['dw'][1], blk['norm'][0], blk['norm'][1], LN_EPS, rowb0, ts[i])
            nv.vc_linear(ts[i], blk['pw1'][0], blk['pw1'][1], 'gelu', None, None, hs[i], rowb0, prec)
            nv.vc_linear(hs[i], blk['pw2'][0], blk['pw2'][1], 'residual', blk['gamma'], xs[i], xs[i + 1], rowb0, prec)
        nv.vc_dwln(xs[L], None, None, pk['final'][0], pk['final'][1], LN_EPS, rowb0, tf)
        nv.vc_linear(tf, pk['head'][0], pk['head'][1], None, None, None, y, rowb0, head_prec)
        nv.vc_polar(y, self.n_fft // 2 + 1, MAG_CLAMP, rowb0, spec)
        nv.vc_linear(spec, pk['basis'], None, None, None, None, frames, rowb0, head_prec)
        nv.vc_ola(frames, pk['wsq'], utt, self.hop, self.trim(), out)
        sv = dict(state=state, mel_cl=mel_cl, e=e, xs=xs, ts=ts, hs=hs, tf=tf, y=y, pk=pk, prec=prec, rowb0=rowb0, rowr0=rowr0,
                  utt=utt, P=P, B=B, N=N, T=T, lens=lens, mel_dtype=mel.dtype, key=self._pack[0])
        return out, sv

    def _packed_t(self, device, pk, key):
        """The transposed weight images of the backward's data-gradient products, built once per weight state: from the
        forward's packed image ``pk`` and under the forward's ``key``."""
        if self._pack_t is not None and self._pack_t[0] == key:
            return self._pack_t[1]
        with torch.no_grad():
            ce, D = _ce(self.n_mel_channels), self.dim
            w = pk['embed'][0].view(D, EMBED_KERNEL, ce)                      # d_mel[r] = sum_t d_e[r - (t - 3)] W[:, t, :]
            pt = dict(basis=pk['basis'].t().contiguous(), head=pk['head'][0].t().contiguous(),
                      embed=w.flip(1).permute(2, 1, 0).reshape(ce, EMBED_KERNEL * D).contiguous(),
                      blocks=[(blk['pw1'][0].t().contiguous(), blk['pw2'][0].t().contiguous()) for blk in pk['blocks']])
        self._pack_t = (key, pt)
        return pt

    def _grad_layout(self, B=0, N=0):
        """(floats, {parameter name: (offset, shape)}) of the flat gradient buffer, every tensor at a multiple of 4 floats; a
        LayerNorm's weight and bias are neighbours (one ordered pass sums both).  'mel' (B, n_mel, N) comes last when asked
        for."""
        lay, o = {}, 0
        for name, p in self.named_parameters():
            lay[name] = (o, tuple(p.shape))
            o += -(-p.numel() // 4) * 4
        if B:
            lay['mel'] = (o, (B, self.n_mel_channels, N))
            o += -(-B * self.n_mel_channels * N // 4) * 4
        return o, lay

    def _bwd_sizes(self, P, B, N, want_mel):
        """Floats of the regions of the backward's one workspace."""
        D, I, L, ce = self.dim, self.intermediate_dim, self.n_fft, _ce(self.n_mel_channels)
        nh, ns, two_f = _pad_cols(L + 2), -(-(L + 2) // 32) * 32, L + 2
        slots = nv.vc_bwd_slots(P)
        M = P - 2 * HALO
        sk = max(_splitk(D, I, P) * D * I, _splitk(two_f, D, P) * two_f * D, _splitk(D, ce, M) * D * ce)
        sizes = dict(d_frames=P * L, d_spec=P * ns, d_y=P * nh, da=P * D, db=P * D, y2=P * D, u=P * I, dh=P * I,
                     partial=slots * (DW_KERNEL + 1) * D, small=(DW_KERNEL + 1) * D, wpart=sk, g_in=D * EMBED_KERNEL * ce,
                     ws64=2 * 2 * 64 * max(I, nh, D), d_mel_cl=P * ce if want_mel else 0, d_mel_rows=B * N * ce if want_mel else 0)
        return {k: -(-v // 4) * 4 for k, v in sizes.items()}

    def _backward(self, sv, d_audio, want_mel):
        """The backward pass over the kept state -> {parameter name (and 'mel'): gradient, a view of one flat buffer}."""
        D, I, L, nm = self.dim, self.intermediate_dim, self.num_layers, self.n_mel_channels
        ce, two_f, F = _ce(nm), self.n_fft + 2, self.n_fft // 2 + 1
        pk, prec, rowb0, rowr0, P, B, N = sv['pk'], sv['prec'], sv['rowb0'], sv['rowr0'], sv['P'], sv['B'], sv['N']
        head_prec = min(prec, 1)
        dev = rowb0.device
        if self._pack_key(dev) != sv['key']:
            raise RuntimeError("Vocos.generate: a parameter was modified between this forward and its backward (an optimiser "
                               "step or an in-place edit); the kept state belongs to the earlier weights")
        pt = self._packed_t(dev, pk, sv['key'])
        d_audio = d_audio.to(device=dev, dtype=torch.float32).contiguous()
        total, lay = self._grad_layout(B if want_mel else 0, N)
        sizes = self._bwd_sizes(P, B, N, want_mel)
        gout = torch.empty(total, dtype=torch.float32, device=dev)
        bw = torch.empty(sum(sizes.values()), dtype=torch.float32, device=dev)
        gv = {name: gout[o:o + int(np.prod(shape))].view(shape) for name, (o, shape) in lay.items()}
        r, o = {}, 0
        for k, n in sizes.items():
            r[k] = bw[o:o + n]
            o += n
        ns = -(-two_f // 32) * 32
        d_frames, d_spec, d_y = r['d_frames'].view(P, self.n_fft), r['d_spec'].view(P, ns), r['d_y'].view(P, -1)
        da, db, y2 = r['da'].view(P, D), r['db'].view(P, D), r['y2'].view(P, D)
        u, dh = r['u'].view(P, I), r['dh'].view(P, I)
        partial, small, wpart, ws64 = r['partial'], r['small'], r['wpart'], r['ws64'].view(torch.float64)
        slots = nv.vc_bwd_slots(P)

        def norm_grads(name):
            o = lay[name + '.weight'][0]
            nv.wg_partial_sum(partial, slots, 2 * D, gout[o:o + 2 * D])

        nv.vc_ola_bwd(d_audio, pk['wsq'], sv['utt'], rowb0, rowr0, self.hop, self.trim(), d_frames)
        nv.vc_linear(d_frames, pt['basis'], None, None, None, None, d_spec, rowb0, head_prec)
        nv.vc_polar_bwd(sv['y'], F, MAG_CLAMP, d_spec, rowb0, d_y)
        _wgrad(gv['head.out.weight'], d_y[:, :two_f], sv['tf'], head_prec, wpart)
        nv.colsum(d_y[:, :two_f], ws64, gv['head.out.bias'])
        nv.vc_linear(d_y, pt['head'], None, None, None, None, db, rowb0, head_prec)
        nv.vc_ln_bwd(sv['xs'][L], None, None, pk['final'][0], LN_EPS, rowb0, db, da, partial)
        norm_grads('backbone.final_layer_norm')
        for i in reversed(range(L)):
            blk, (w1t, w2t), pre = pk['blocks'][i], pt['blocks'][i], 'backbone.convnext.%d.' % i
            x, t, h = sv['xs'][i], sv['ts'][i], sv['hs'][i]
            # da = the gradient of the block's output; the residual passes it on, gamma scales it into pwconv2
            nv.vc_linear(h, blk['pw2'][0], blk['pw2'][1], None, None, None, y2, rowb0, prec)
            nv.vc_gamma_bwd(da, blk['gamma'], rowb0, y2, partial)
            nv.wg_partial_sum(partial, slots, D, gv[pre + 'gamma'])
            _wgrad(gv[pre + 'pwconv2.weight'], y2, h, prec, wpart)
            nv.colsum(y2, ws64, gv[pre + 'pwconv2.bias'])
            nv.vc_linear(y2, w2t, None, None, None, None, dh, rowb0, prec)
            nv.vc_linear(t, blk['pw1'][0], blk['pw1'][1], None, None, None, u, rowb0, prec)
            nv.vc_gelu_bwd(u, rowb0, dh)
            _wgrad(gv[pre + 'pwconv1.weight'], dh, t, prec, wpart)
            nv.colsum(dh, ws64, gv[pre + 'pwconv1.bias'])
            nv.vc_linear(dh, w1t, None, None, None, None, db, rowb0, prec)
            nv.vc_ln_bwd(x, blk['dw'][0], blk['dw'][1], blk['norm'][0], LN_EPS, rowb0, db, db, partial)
            norm_grads(pre + 'norm')
            nv.vc_dw_bwd(db, x, blk['dw'][0], rowb0, da, da, partial)
            nv.wg_partial_sum(partial, slots, (DW_KERNEL + 1) * D, small[:(DW_KERNEL + 1) * D])
            gv[pre + 'dwconv.weight'].view(D, DW_KERNEL).copy_(small[:DW_KERNEL * D].view(DW_KERNEL, D).t())
            gv[pre + 'dwconv.bias'].copy_(small[DW_KERNEL * D:(DW_KERNEL + 1) * D])
        nv.vc_ln_bwd(sv['e'], None, None, pk['norm'][0], LN_EPS, rowb0, da, db, partial)
        norm_grads('backbone.norm')
        # embed: its 7 taps are 7 shifted row slices of the zero-haloed mel image
        d_e, mel_cl = db, sv['mel_cl']
        g_in = r['g_in'][:D * EMBED_KERNEL * ce].view(D, EMBED_KERNEL * ce)
        for tap in range(EMBED_KERNEL):
            _wgrad(g_in[:, tap * ce:(tap + 1) * ce], d_e[HALO:P - HALO], mel_cl[tap:P - 2 * HALO + tap], prec, wpart)
        gv['backbone.embed.weight'].copy_(g_in.view(D, EMBED_KERNEL, ce)[:, :, :nm].permute(0, 2, 1))
        nv.colsum(d_e, ws64, gv['backbone.embed.bias'])
        if want_mel:
            d_mel_cl = r['d_mel_cl'][:P * ce].view(P, ce)
            rows = r['d_mel_rows'][:B * N * ce].view(B * N, ce)
            nv.hg_conv(d_e, pt['embed'], None, EMBED_KERNEL, 1, None, None, d_mel_cl, 1.0, False, rowb0, 1, prec)
            torch.index_select(d_mel_cl, 0, self._mel_rows(sv['lens'], N, dev), out=rows)     # row 0 is a halo row: zero
            gv['mel'].copy_(rows.view(B, N, ce)[:, :, :nm].transpose(1, 2))
        return gv

    def _mel_rows(self, lens, N, dev):
        """(B N) int64: the packed row of frame n of utterance b, row 0 (a halo row) beyond its frames."""
        key = ('mel_rows', tuple(lens), N, str(dev))
        if getattr(self, '_mel_rows_cache', None) is None or self._mel_rows_cache[0] != key:
            offs = self.packed_plan(lens)[3]
            idx = torch.zeros(len(lens), N, dtype=torch.int64)
            for b, (o, n) in enumerate(zip(offs, lens)):
                idx[b, :n] = torch.arange(o, o + n)
            self._mel_rows_cache = (key, idx.view(-1).to(dev))
        return self._mel_rows_cache[1]


class _Generate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vc, mel, lengths, *params):
        out, sv = vc._generate_forward(mel, lengths)
        ctx.vc, ctx.sv = vc, sv
        ctx.names = [n for n, _ in vc.named_parameters()]
        return out

    @staticmethod
    def backward(ctx, d_audio):
        if ctx.sv is None:
            raise RuntimeError("Vocos.generate: backward was already run; the kept state is freed by the first one")
        want_mel = ctx.needs_input_grad[1]
        gv = ctx.vc._backward(ctx.sv, d_audio, want_mel)
        mel_dtype = ctx.sv['mel_dtype']
        ctx.sv = None
        return (None, gv['mel'].to(mel_dtype) if want_mel else None, None) + \
            tuple(gv[n] if need else None for n, need in zip(ctx.names, ctx.needs_input_grad[3:]))


def load_vocos(src, precision=None, hop_length=None, padding=None):
    """A Vocos from a checkpoint path, a state dict, ``{'state_dict': state dict}`` or a module.  ``precision`` defaults to
    'fp32', ``hop_length`` to n_fft / 4, ``padding`` to 'same'.  A Vocos instance is returned as it is, with ``precision``
    set when given; a hop or padding other than its own is refused (they are part of its geometry)."""
    src = checkpoint_source(src, 'state_dict')
    if isinstance(src, Vocos):
        if (hop_length is not None and int(hop_length) != src.hop) or (padding is not None and padding != src.padding):
            raise ValueError("load_vocos: the module has hop %d and padding %r, asked for hop %s and padding %r"
                             % (src.hop, src.padding, hop_length, padding))
        if precision is not None:
            src.precision = precision
        return src
    precision = 'fp32' if precision is None else precision
    padding = 'same' if padding is None else padding
    return Vocos._from_source(src, "load_vocos", precision=precision, hop_length=hop_length, padding=padding)
