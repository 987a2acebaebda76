"""WaveGlow inference on the MI355X: NVIDIA's vocoder (glow.py, the reference notebook's ``waveglow.infer`` and
denoiser.py's ``Denoiser``) as native HIP passes.

    wg = load_waveglow("waveglow.pt").cuda().eval()
    audio = wg.infer(mel, sigma=0.666)                 # (B, 256 * N) float32
    clean = Denoiser(wg)(audio, strength=0.01)         # (B, 1, T)
    z, log_s_list, log_det_W_list = wg((mel, audio))   # glow.py's forward: audio -> latents (no grad: see training_loss)
    nats = wg.nll(mel, audio, sigma=1.0)               # (B,) negative log-likelihood per sample, per utterance
    loss = wg.training_loss(mel, audio, sigma=1.0)     # float32 scalar with a grad_fn; loss.backward() fills p.grad
    wg.apply_weight_norm()                             # glow.py's training parametrisation: weight_g / weight_v

The module keeps NVIDIA's submodule names (after ``remove_weightnorm``), so ``state_dict()`` keys match glow.py.  Its
weights are f32 masters; ``precision`` selects the compute of the products: 'fp32' (exact f32 MFMA), 'bf16x3'
(split-bf16, three products) or 'bf16'.  ``.half()`` keeps the f32 weights, selects 'bf16' and makes ``infer`` return
float16; ``.float()`` goes back to 'fp32'.

Per call: one upsample product per utterance, then per flow one cond product (t2amd_gemm_f32), two WN layer products per
layer (t2amd_wg_layer_f32: the gated dilated product and the residual / skip product) and one flow tail
(t2amd_wg_tail_f32: end, affine inverse, inverse 1x1 mix, noise insertion and the next flow's start).  All buffers are
allocated once per call, before the flow loop, which does no allocation, copy or host synchronisation.
The forward direction (``forward``, ``nll``, ``WaveGlowLoss``) runs the same products; between them one flow head per
flow boundary (t2amd_wg_head_f32: end, affine coupling, log_s, early output, the next flow's 1x1 mix and start) and, for
the loss, one fixed-order reduction (t2amd_wg_nll_f32).  ``forward`` has no backward pass: its outputs do not require grad.
Training goes through ``training_loss``, a torch.autograd.Function over the module's parameters: the same launches with
the state the backward pass needs kept in one allocation, then per flow boundary one head backward
(t2amd_wg_head_bwd_f32), per layer one gate backward, the data gradient in one launch (mode 2 of the layer product) and
the weight gradients on split-K t2amd_gemm_f32.
Under weight norm (``WaveGlow(weight_norm=True)`` / ``apply_weight_norm``: glow.py's own training parametrisation, the keys
of NVIDIA's training checkpoints) start, in_layers, res_skip_layers and cond_layer own ``weight_g`` / ``weight_v``; all of
them are folded into one flat buffer by one launch per weight version (t2amd_wg_weight_norm_f32) and their gradients
come from one more launch per backward pass (t2amd_wg_weight_norm_bwd_f32); everything else is the folded module's path.
The arithmetic is restated in float64 torch by tests/waveglow_ref.py and tests/waveglow_fwd_ref.py; DESIGN.md section 10
has the layout.
"""

import numpy as np
import torch
from torch import nn

from . import native as nv
from .audio import STFT
from .vocoder import PRECISIONS, Vocoder, checkpoint_source, host_lengths, packed_rows, _splitk, _wgrad

HOP = 256                    # upsample stride (NVIDIA's ConvTranspose1d(n_mel, n_mel, 1024, stride=256))
UP_KERNEL = 1024


def fold_weight_norm(state_dict):
    """Replace every ``X.weight_g`` / ``X.weight_v`` pair by ``X.weight = g * v / ||v||`` (norm over all dims but 0),
    computed as ``torch.nn.utils.remove_weight_norm`` does."""
    out = {}
    for k, v in state_dict.items():
        if k.endswith('.weight_v'):
            continue
        if k.endswith('.weight_g'):
            base = k[:-len('_g')]
            out[base] = torch._weight_norm(state_dict[base + '_v'], v, 0).detach()
        else:
            out[k] = v
    return out


def config_from_state_dict(state_dict):
    """WaveGlow constructor arguments from the tensor shapes of a (folded or weight-normed) state dict."""
    sd = state_dict
    legacy = [k for k in sd if '.cond_layers.' in k or '.res_layers.' in k or '.skip_layers.' in k]
    if legacy:
        raise ValueError("WaveGlow: this is the pre-2019 checkpoint layout (per-layer cond_layers, separate res_layers / "
                         "skip_layers, e.g. %s); convert it with NVIDIA's convert_model.py first" % legacy[0])

    def w(name):
        for suffix in ('.weight', '.weight_v'):
            if name + suffix in sd:
                return sd[name + suffix]
        raise KeyError("WaveGlow: missing %s.weight" % name)

    flows = sorted({int(k.split('.')[1]) for k in sd if k.startswith('WN.')})
    if not flows or flows != list(range(len(flows))):
        raise ValueError("WaveGlow: no WN.<k> flows in the state dict")
    n_flows = len(flows)
    n_mel = w('upsample').shape[0]
    C = w('WN.0.start').shape[0]
    L = len({k.split('.')[3] for k in sd if k.startswith('WN.0.in_layers.')})
    ks = w('WN.0.in_layers.0').shape[2]
    chans = [w('convinv.%d.conv' % k).shape[0] for k in range(n_flows)]
    n_group = chans[0]
    every, size = n_flows, 0
    for k in range(1, n_flows):
        if chans[k] != chans[0]:
            every, size = k, chans[0] - chans[k]
            break
    cfg = dict(n_mel_channels=n_mel, n_flows=n_flows, n_group=n_group, n_early_every=every, n_early_size=size,
               WN_config=dict(n_layers=L, n_channels=C, kernel_size=ks))
    want, c = [], n_group
    for k in range(n_flows):
        if k % every == 0 and k > 0:
            c -= size
        want.append(c)
    if want != chans:
        raise ValueError("WaveGlow: per-flow channel counts %s follow no (n_early_every, n_early_size)" % chans)
    return cfg


class Invertible1x1Conv(nn.Module):
    """glow.py's Invertible1x1Conv: a bias-free 1x1 conv with an orthonormal, det = +1 initial weight.  Only the
    inverse is used at inference (computed once per weight version in float64, see WaveGlow._packed)."""

    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv1d(c, c, kernel_size=1, stride=1, padding=0, bias=False)
        W = torch.linalg.qr(torch.randn(c, c))[0]
        if torch.det(W) < 0:
            W[:, 0] = -W[:, 0]
        self.conv.weight.data = W.contiguous().view(c, c, 1)


class WN(nn.Module):
    """glow.py's WN (the fused-cond form): start, in_layers, res_skip_layers, cond_layer, end."""

    def __init__(self, n_in_channels, n_mel_channels, n_layers, n_channels, kernel_size):
        super().__init__()
        self.n_layers, self.n_channels = n_layers, n_channels
        self.in_layers = nn.ModuleList()
        self.res_skip_layers = nn.ModuleList()
        self.start = nn.Conv1d(n_in_channels, n_channels, 1)
        self.end = nn.Conv1d(n_channels, 2 * n_in_channels, 1)
        self.end.weight.data.zero_()                  # NVIDIA's init: every affine coupling starts as the identity
        self.end.bias.data.zero_()
        self.cond_layer = nn.Conv1d(n_mel_channels, 2 * n_channels * n_layers, 1)
        for i in range(n_layers):
            d = 2 ** i
            self.in_layers.append(nn.Conv1d(n_channels, 2 * n_channels, kernel_size, dilation=d,
                                            padding=(kernel_size * d - d) // 2))
            self.res_skip_layers.append(nn.Conv1d(n_channels, 2 * n_channels if i < n_layers - 1 else n_channels, 1))


class WaveGlow(Vocoder):
    LABEL = 'WaveGlow'

    def __init__(self, n_mel_channels, n_flows, n_group, n_early_every, n_early_size, WN_config, precision='fp32',
                 weight_norm=False):
        super().__init__()
        C, L, ks = WN_config['n_channels'], WN_config['n_layers'], WN_config['kernel_size']
        if ks != 3:
            raise ValueError("WaveGlow: kernel_size %d is not supported (the native path is kernel 3)" % ks)
        if n_group % 2:
            raise ValueError("WaveGlow: n_group must be even, got %d" % n_group)
        if n_group > 16 or HOP % n_group:
            raise ValueError("WaveGlow: n_group must divide %d and be at most 16, got %d" % (HOP, n_group))
        if C % 64 or C > 512:
            raise ValueError("WaveGlow: n_channels must be a multiple of 64 up to 512, got %d" % C)
        if n_early_size % 2:
            raise ValueError("WaveGlow: n_early_size must be even, got %d" % n_early_size)
        if n_mel_channels % 16:
            raise ValueError("WaveGlow: n_mel_channels must be a multiple of 16, got %d" % n_mel_channels)
        self.n_mel_channels, self.n_flows, self.n_group = n_mel_channels, n_flows, n_group
        self.n_early_every, self.n_early_size = n_early_every, n_early_size
        self.n_layers, self.n_channels = L, C
        self.upsample = nn.ConvTranspose1d(n_mel_channels, n_mel_channels, UP_KERNEL, stride=HOP)
        self.WN = nn.ModuleList()
        self.convinv = nn.ModuleList()
        n_half, n_rem = n_group // 2, n_group
        self.flow_channels = []
        for k in range(n_flows):
            if k % n_early_every == 0 and k > 0:
                n_half -= n_early_size // 2
                n_rem -= n_early_size
            if n_rem < 2:
                raise ValueError("WaveGlow: the early outputs leave %d channels" % n_rem)
            self.convinv.append(Invertible1x1Conv(n_rem))
            self.WN.append(WN(n_half, n_mel_channels * n_group, **WN_config))
            self.flow_channels.append(n_rem)
        self.n_remaining_channels = n_rem
        self.precision = precision
        self.weight_norm = False
        self._wn = None
        if weight_norm:
            self.apply_weight_norm()

    # ---- loading ------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True, assign=False):
        """A folded module folds a weight-normed state dict on load; a weight-normed module takes ``weight_g`` /
        ``weight_v`` as they are and refuses a folded state dict."""
        sd = dict(state_dict)
        if self.weight_norm:
            if not any(k.endswith('.weight_g') for k in sd):
                raise ValueError("WaveGlow: the module is weight-normed (weight_g / weight_v) and the state dict is folded: "
                                 "load it into a folded module and call apply_weight_norm(), or remove_weight_norm() first")
        else:
            sd = fold_weight_norm(sd)
        cfg = config_from_state_dict(sd)
        mine = dict(n_mel_channels=self.n_mel_channels, n_flows=self.n_flows, n_group=self.n_group,
                    WN_config=dict(n_layers=self.n_layers, n_channels=self.n_channels, kernel_size=3))
        got = {k: cfg[k] for k in mine}
        if got != mine:
            raise ValueError("WaveGlow: state dict geometry %s does not match the module's %s" % (got, mine))
        self._pack = None
        return super().load_state_dict(self._f32_state(sd), strict=strict, assign=assign)

    @classmethod
    def from_state_dict(cls, state_dict, precision='fp32', weight_norm=False):
        """``weight_norm=False`` (default) folds ``weight_g`` / ``weight_v``; ``weight_norm=True`` gives a weight-normed
        module that keeps them as they are (a folded source gets ``v = w``, ``g = ||w||``)."""
        sd = dict(state_dict)
        if weight_norm and any(k.endswith('.weight_g') for k in sd):
            m = cls(precision=precision, weight_norm=True, **config_from_state_dict(sd))
            m.load_state_dict(sd)
            return m
        sd = fold_weight_norm(sd)
        m = cls(precision=precision, **config_from_state_dict(sd))
        m.load_state_dict(sd)
        return m.apply_weight_norm() if weight_norm else m

    # ---- the g / v parametrisation ------------------------------------------------------------------------------------
    def _wn_modules(self):
        """(name, conv) of the layers glow.py wraps in weight norm, in table order."""
        for k, wn in enumerate(self.WN):
            pre = 'WN.%d.' % k
            yield pre + 'start', wn.start
            for i in range(self.n_layers):
                yield pre + 'in_layers.%d' % i, wn.in_layers[i]
            for i in range(self.n_layers):
                yield pre + 'res_skip_layers.%d' % i, wn.res_skip_layers[i]
            yield pre + 'cond_layer', wn.cond_layer

    def _folded_shapes(self):
        """[(name, shape)] of the parameters of the folded form, in ``named_parameters`` order."""
        out = []
        for name, p in self.named_parameters():
            if name.endswith('.weight_g'):
                continue
            out.append((name[:-2], tuple(p.shape)) if name.endswith('.weight_v') else (name, tuple(p.shape)))
        return out

    def apply_weight_norm(self):
        """Switch to glow.py's training parametrisation in place: start, in_layers, res_skip_layers and cond_layer of
        every flow own ``weight_g`` (C_out, 1, 1) and ``weight_v`` instead of ``weight``, with ``v = w`` and ``g = ||w||``
        per output channel (what ``torch.nn.utils.weight_norm`` does), so the function computed does not change.
        ``state_dict()`` then has the keys of NVIDIA's training checkpoints."""
        if self.weight_norm:
            return self
        with torch.no_grad():
            for _, m in self._wn_modules():
                w = m.weight
                g = nn.Parameter(torch.norm_except_dim(w.detach(), 2, 0), requires_grad=w.requires_grad)
                v = nn.Parameter(w.detach().clone(), requires_grad=w.requires_grad)
                del m._parameters['weight']
                m.register_parameter('weight_g', g)
                m.register_parameter('weight_v', v)
                m.weight = w.detach()                  # a plain attribute from here on: a slice of the fold's output
        self.weight_norm, self._pack = True, None
        self._wn_flatten()
        return self

    def remove_weight_norm(self):
        """Back to the folded form in place: ``weight = g v / ||v||``, computed as ``torch.nn.utils.remove_weight_norm``
        does (``fold_weight_norm``)."""
        if not self.weight_norm:
            return self
        with torch.no_grad():
            for _, m in self._wn_modules():
                g, v = m.weight_g, m.weight_v
                w = nn.Parameter(torch._weight_norm(v.detach(), g.detach(), 0), requires_grad=v.requires_grad)
                del m._parameters['weight_g'], m._parameters['weight_v']
                m.__dict__.pop('weight', None)
                m.register_parameter('weight', w)
        self.weight_norm, self._wn, self._pack = False, None, None
        return self

    @staticmethod
    def remove_weightnorm(model):
        """glow.py's spelling: ``WaveGlow.remove_weightnorm(model)`` returns the folded model."""
        return model.remove_weight_norm()

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        if getattr(self, 'weight_norm', False):
            self._wn_flatten()                         # .cuda() / .to() gave every parameter an allocation of its own
        return self

    def _wn_flatten(self):
        """Lay all ``weight_v`` out in one flat buffer and all ``weight_g`` in another (the parameters become views of
        them, keeping their identity), beside the buffers of the folded weights and the norms, and build the segment table
        of csrc/waveglow_wn.hip once.  Tensors start at multiples of 4 floats, so rows of a multiple of 4 floats move
        as 16-byte accesses."""
        mods = list(self._wn_modules())
        dev = mods[0][1].weight_v.device
        _, glay, _ = self._grad_layout()
        lay, segs, off, goff = [], [], 0, 0
        for name, m in mods:
            shape = tuple(m.weight_v.shape)
            rows, ln = shape[0], int(np.prod(shape[1:]))
            lay.append((name, m, off, goff, shape))
            segs.append((off, goff, glay[name + '.weight'][0], rows, ln))
            off = -(-(off + rows * ln) // 4) * 4
            goff += rows
        host, n_units = nv.wg_weight_norm_table(segs)
        v = torch.zeros(off, dtype=torch.float32, device=dev)
        g = torch.zeros(-(-goff // 4) * 4, dtype=torch.float32, device=dev)
        w, norm = torch.zeros_like(v), torch.zeros_like(g)
        with torch.no_grad():
            for name, m, o, go, shape in lay:
                n = int(np.prod(shape))
                vv, gg = v[o:o + n].view(shape), g[go:go + shape[0]].view(shape[0], 1, 1)
                vv.copy_(m.weight_v.detach())
                gg.copy_(m.weight_g.detach())
                m.weight_v.data, m.weight_g.data = vv, gg
                m.weight = w[o:o + n].view(shape)
        self._wn = dict(dev=dev, v=v, g=g, w=w, norm=norm, host=host, table=host.to(dev), n_units=n_units, lay=lay)
        self._pack = None

    def _wn_fold(self):
        """One launch: the folded weights of every weight-normed layer, into the buffer ``module.weight`` is a slice of."""
        wn = self._wn
        stale = wn is None or any(m.weight_v.data_ptr() != wn['v'].data_ptr() + 4 * o
                                  or m.weight_g.data_ptr() != wn['g'].data_ptr() + 4 * go for _, m, o, go, _ in wn['lay'])
        if stale:                                      # parameters replaced behind the module's back (assign=True, deepcopy)
            self._wn_flatten()
            wn = self._wn
        nv.wg_weight_norm(wn['table'], wn['host'], wn['n_units'], wn['v'], wn['g'], wn['w'], wn['norm'])

    def _wn_grads(self, gout, gv):
        """One launch: the gradients of every ``weight_g`` / ``weight_v`` from the folded weights' gradients in ``gout``
        (already times the upstream scalar), added to ``gv`` under the parameters' names."""
        wn = self._wn
        nvf, ngf = wn['v'].numel(), wn['g'].numel()
        buf = torch.empty(nvf + ngf, dtype=torch.float32, device=gout.device)
        dv, dg = buf[:nvf], buf[nvf:]
        nv.wg_weight_norm_bwd(wn['table'], wn['host'], wn['n_units'], gout, wn['v'], wn['g'], wn['norm'], dg, dv, 1.0)
        for name, _, o, go, shape in wn['lay']:
            gv[name + '.weight_v'] = dv[o:o + int(np.prod(shape))].view(shape)
            gv[name + '.weight_g'] = dg[go:go + shape[0]].view(shape[0], 1, 1)

    # ---- device-side weight layout ------------------------------------------------------------------------------------
    def _packed(self, device):
        key = self._pack_key(device)
        if self._pack is not None and self._pack[0] == key:
            return self._pack[1]
        if self.weight_norm:
            self._wn_fold()
            key = self._pack_key(device)
        C, L, G, nm = self.n_channels, self.n_layers, self.n_group, self.n_mel_channels
        taps = UP_KERNEL // HOP
        with torch.no_grad():
            # upsample: out[q][p n_mel + co] = sum_{j, ci} x[q - j][ci] W[ci][co][p + 256 j]  (B operand [N][K], K = (j, ci))
            W = self.upsample.weight.detach().float().view(nm, nm, taps, HOP)
            up_w = W.permute(3, 1, 2, 0).reshape(HOP * nm, taps * nm).contiguous()
            up_b = self.upsample.bias.detach().float().repeat(HOP).contiguous()
            # gate packing: block 64 q + [0, 32) = tanh channels 32 q + [0, 32), block 64 q + [32, 64) their partners
            q = torch.arange(C // 32).view(-1, 1, 1)
            half = torch.arange(2).view(1, -1, 1)
            j = torch.arange(32).view(1, 1, -1)
            gate_perm = (half * C + 32 * q + j).reshape(-1).to(device)
            flows, logdet = [], []
            for k in range(self.n_flows):
                wn = self.WN[k]
                f = {}
                cw = wn.cond_layer.weight.detach().float().view(2 * C * L, nm, G)
                f['cond_w'] = cw.permute(0, 2, 1).reshape(2 * C * L, G * nm).contiguous()     # column g n_mel + c
                f['cond_b'] = wn.cond_layer.bias.detach().float().contiguous()
                f['in_w'], f['in_b'], f['rs_w'], f['rs_b'], f['in_wT'] = [], [], [], [], []
                for i in range(L):
                    iw = wn.in_layers[i].weight.detach().float().permute(0, 2, 1).reshape(2 * C, 3 * C)
                    # the data gradient's operand: [c][tap' 2C + n] = W[n][c][2 - tap'] (channel order, taps mirrored)
                    f['in_wT'].append(wn.in_layers[i].weight.detach().float().flip(2).permute(1, 2, 0)
                                      .reshape(C, 6 * C).contiguous())
                    f['in_w'].append(iw.index_select(0, gate_perm).contiguous())
                    f['in_b'].append(wn.in_layers[i].bias.detach().float().index_select(0, gate_perm).contiguous())
                    rw = wn.res_skip_layers[i].weight.detach().float()
                    f['rs_w'].append(rw.view(rw.shape[0], C).contiguous())
                    f['rs_b'].append(wn.res_skip_layers[i].bias.detach().float().contiguous())
                sw = wn.start.weight.detach().float()
                f['start_w'] = sw.view(C, sw.shape[1]).contiguous()
                f['start_b'] = wn.start.bias.detach().float().contiguous()
                ew = wn.end.weight.detach().float()
                f['end_w'] = ew.view(ew.shape[0], C).contiguous()
                f['end_b'] = wn.end.bias.detach().float().contiguous()
                wc = self.convinv[k].conv.weight.detach()
                winv64 = torch.linalg.inv(wc.double().cpu().view(wc.shape[0], wc.shape[0]))
                f['winv'] = winv64.float().contiguous().to(device)
                # d(-sum_b T'_b log det W) / dW / numel = -W^-T / n_group, whatever the batch
                f['mix_ldg'] = (-winv64.t() / G).float().contiguous().to(device)
                # the forward direction: the weight itself and log det W (float64 on the host; nan when det W < 0, as
                # torch.logdet gives)
                f['mix_w'] = wc.float().view(wc.shape[0], wc.shape[0]).contiguous()
                sign, logabs = torch.linalg.slogdet(wc.double().cpu().view(wc.shape[0], wc.shape[0]))
                logdet.append(float(logabs) if float(sign) > 0 else (float('-inf') if float(sign) == 0 else float('nan')))
                flows.append(f)
        pk = dict(up_w=up_w, up_b=up_b, flows=flows, logdet=logdet)
        self._pack = (key, pk)
        return pk

    # ---- inference ----------------------------------------------------------------------------------------------------
    def halo(self):
        return 2 ** (self.n_layers - 1)            # (kernel_size - 1) / 2 * the deepest dilation

    def noise_shapes(self, B, N):
        """Shapes of the noise tensors infer draws, in draw order (reference: FloatTensor(...).normal_())."""
        R = HOP * N // self.n_group
        shapes = [(B, self.n_remaining_channels, R)]
        for k in reversed(range(self.n_flows)):
            if k % self.n_early_every == 0 and k > 0:
                shapes.append((B, self.n_early_size, R))
        return shapes

    def packed_plan(self, lengths):
        """(rowb, rowr, offsets, P) of the packed row space for per-utterance frame counts `lengths` (host tensors)."""
        return packed_rows([HOP // self.n_group * int(n) for n in lengths], self.halo())

    def _plan(self, dev, rows, frames=None):
        """(rowb, rowr on the device, offsets, P): ``packed_plan(rows)``, or with ``frames`` ``forward_plan(rows, frames)``,
        built and uploaded once while the same direction, lengths and device repeat.  The cache, the caller and the state
        kept for a backward pass hold the same tensors and the same list: read-only for all of them."""
        def build():
            rowb, rowr, offs, P = self.packed_plan(rows) if frames is None else self.forward_plan(rows, frames)
            return rowb.to(dev), rowr.to(dev), offs, P
        return self._cached_plan((frames is None, tuple(rows), None if frames is None else tuple(frames), str(dev)), build)

    def _workspace(self, P, B, N, dev):
        """One allocation per call: cond_g [P][G n_mel] (zeroed) | cnd [P][2CL] | h (zeroed), acts, skip [P][C] |
        audio [P][G] | mel_cl [B N][n_mel]."""
        C, L, G, nm = self.n_channels, self.n_layers, self.n_group, self.n_mel_channels
        widths = [G * nm, 2 * C * L, C, C, C, G]
        ws = torch.empty(P * sum(widths) + B * N * nm, dtype=torch.float32, device=dev)
        cond_g, cnd, h, acts, skip, audio = self._regions(ws, P, widths)
        mel_cl = ws[P * sum(widths):].view(B * N, nm)
        cond_g.zero_()
        h.zero_()
        return cond_g, cnd, h, acts, skip, audio, mel_cl

    @torch.no_grad()
    def infer(self, spect, sigma=1.0, lengths=None, z=None):
        """(B, n_mel, N) mels (float32 / float16 / bfloat16) -> (B, 256 N) audio (float16 after ``.half()``).
        ``lengths``: frames per utterance (ragged: each computed as if alone, zero beyond 256 n_b); ``z``: the noise
        tensors in ``noise_shapes`` order instead of drawing them."""
        dev = self._device()
        B, nm, N, lens = self._check_mels(spect, lengths, "infer")
        shapes = self.noise_shapes(B, N)
        if z is None:
            z = [torch.empty(s, dtype=torch.float32, device=dev).normal_() for s in shapes]
        else:
            z = list(z)
            if [tuple(t.shape) for t in z] != shapes:
                raise ValueError("WaveGlow.infer: noise shapes %s, expected %s" % ([tuple(t.shape) for t in z], shapes))
            z = [t.to(device=dev, dtype=torch.float32).contiguous() for t in z]
        prec = PRECISIONS[self.precision]
        pk = self._packed(dev)
        C, L, G, H = self.n_channels, self.n_layers, self.n_group, self.halo()
        rowb, rowr, offs, P = self._plan(dev, lens)
        mel = spect.to(device=dev, dtype=torch.float32).contiguous()

        cond_g, cnd, h, acts, skip, audio, mel_cl = self._workspace(P, B, N, dev)
        out = torch.zeros(B, HOP * N, dtype=torch.float32, device=dev)

        # upsample + grouping: one implicit-conv product per utterance, rows straight into the packed space
        nv.transpose(mel_cl[:N], mel[0], batch=B, sstride=nm * N, dstride=N * nm)
        taps = UP_KERNEL // HOP
        spf = HOP // G
        for b, n in enumerate(lens):
            dst = cond_g[offs[b]:offs[b] + spf * n].view(n, HOP * nm)
            nv.gemm(dst, mel_cl[b * N:b * N + n], pk['up_w'], bias=pk['up_b'], convA=(n, nm, 0, -1), fast=prec)

        rows = slice(H, P - H)
        cond_r, cnd_r, h_r, acts_r, skip_r, rowb_r = cond_g[rows], cnd[rows], h[rows], acts[rows], skip[rows], rowb[rows]
        fl = pk['flows']
        nv.wg_tail(rowb, rowr, audio, G, z=z[0], sigma=sigma, start_w=fl[-1]['start_w'], start_b=fl[-1]['start_b'], h=h)
        zi = 1
        for k in reversed(range(self.n_flows)):
            f = fl[k]
            nv.gemm(cnd_r, cond_r, f['cond_w'], bias=f['cond_b'], fast=prec)
            for i in range(L):
                nv.wg_gated(h_r, f['in_w'][i], f['in_b'][i], 2 ** i, cnd_r[:, 2 * C * i:2 * C * (i + 1)], acts_r, prec)
                last = i == L - 1
                nv.wg_res_skip(acts_r, f['rs_w'][i], f['rs_b'][i], None if last else h_r, skip_r, i == 0, rowb_r, prec)
            early = k % self.n_early_every == 0 and k > 0
            nxt = fl[k - 1] if k > 0 else None
            nv.wg_tail(rowb, rowr, audio, G, skip=skip, end_w=f['end_w'], end_b=f['end_b'], winv=f['winv'],
                       z=z[zi] if early else None, sigma=sigma,
                       start_w=nxt['start_w'] if nxt else None, start_b=nxt['start_b'] if nxt else None,
                       h=h if nxt else None, out=out if k == 0 else None)
            zi += 1 if early else 0
        return self._io(out)

    # ---- forward direction: audio -> latents ----------------------------------------------------------------------------
    def early_outputs(self):
        """The flows k > 0 that are preceded by an early output."""
        return [k for k in range(1, self.n_flows) if k % self.n_early_every == 0]

    def latents_to_noise(self, z):
        """(B, n_group, T') latents of ``forward`` -> the noise list ``infer(z=...)`` takes (``noise_shapes`` order): the
        remaining channels first, then the early outputs in reverse order."""
        E, n_e = self.n_early_size, len(self.early_outputs())
        return [z[:, E * n_e:]] + [z[:, E * i:E * (i + 1)] for i in reversed(range(n_e))]

    def noise_to_latents(self, noise):
        """The inverse of ``latents_to_noise``."""
        noise = list(noise)
        if len(noise) != len(self.early_outputs()) + 1:
            raise ValueError("WaveGlow.noise_to_latents: %d tensors, expected %d" % (len(noise), len(self.early_outputs()) + 1))
        return torch.cat(noise[:0:-1] + noise[:1], 1)

    def forward_plan(self, rows, frames):
        """(rowb, rowr, offsets, P) of the packed row space of the forward direction: utterance b holds ``rows[b]`` real rows
        in a slot of ``frames[b]`` whole mel frames (hop / n_group rows each, what the upsample product writes); the rows of
        the last partial frame beyond ``rows[b]`` are marked like halo rows, so they are never computed into h or read back."""
        return packed_rows(rows, self.halo(), [HOP // self.n_group * int(nf) for nf in frames])

    def _forward(self, spect, audio, lengths, who, save=False):
        """-> (z (B, n_group, T') f32, log_s of all flows (B, sum_k n_half_k, T') f32, rows per utterance (host list),
        the state kept for the backward pass (``save``) or None)."""
        dev = self._device()
        B, nm, N, _ = self._check_mels(spect, None, who)
        if not torch.is_tensor(audio) or audio.dim() != 2 or audio.shape[0] != B:
            raise ValueError("WaveGlow.%s: expected (B, T) audio for %d mels, got %s"
                             % (who, B, tuple(audio.shape) if torch.is_tensor(audio) else type(audio)))
        if audio.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError("WaveGlow.%s: audio must be float32, float16 or bfloat16, got %s" % (who, audio.dtype))
        T = audio.shape[1]
        C, L, G, H = self.n_channels, self.n_layers, self.n_group, self.halo()
        lens = host_lengths(lengths, B, T)
        if len(lens) != B or min(lens) < 1 or max(lens) > T:
            raise ValueError("WaveGlow.%s: lengths %s do not fit %d utterances of %d samples" % (who, lens, B, T))
        if any(t % G for t in lens):
            raise ValueError("WaveGlow.%s: the sample counts %s must be multiples of n_group = %d (trim the audio; glow.py "
                             "drops the remainder silently)" % (who, sorted({t for t in lens if t % G}), G))
        if max(lens) > HOP * N:
            raise ValueError("WaveGlow.%s: %d samples need more than the %d mel frames given: T must be at most 256 * N = %d"
                             % (who, max(lens), N, HOP * N))
        Rm = T // G
        rows = [t // G for t in lens]
        frames = [-(-t // HOP) for t in lens]             # mel frames at or past ceil(T_b / 256) cannot reach the audio
        prec = PRECISIONS[self.precision]
        pk = self._packed(dev)
        rowb, rowr, offs, P = self._plan(dev, rows, frames)
        mel = spect.to(device=dev, dtype=torch.float32).contiguous()
        wav = audio.to(device=dev, dtype=torch.float32).contiguous()

        cond_g, cnd, h, acts, skip, a_rows, mel_cl = self._workspace(P, B, N, dev)
        sv = _SavedState(self, P, sum(frames), dev) if save else None
        n_halves = [c // 2 for c in self.flow_channels]
        z = torch.zeros(B, G, Rm, dtype=torch.float32, device=dev)
        log_s = torch.zeros(B, sum(n_halves), Rm, dtype=torch.float32, device=dev)

        # upsample + grouping, trimmed at the front: whole frames into the utterance's own slot of the packed space
        nv.transpose(mel_cl[:N], mel[0], batch=B, sstride=nm * N, dstride=N * nm)
        spf = HOP // G
        for b, nf in enumerate(frames):
            dst = cond_g[offs[b]:offs[b] + spf * nf].view(nf, HOP * nm)
            nv.gemm(dst, mel_cl[b * N:b * N + nf], pk['up_w'], bias=pk['up_b'], convA=(nf, nm, 0, -1), fast=prec)

        inner = slice(H, P - H)
        cond_r, cnd_r, h_r, acts_r, skip_r, rowb_r = cond_g[inner], cnd[inner], h[inner], acts[inner], skip[inner], rowb[inner]
        fl = pk['flows']
        if sv is None:
            nv.wg_head(rowb, rowr, a_rows, G, B, Rm, wave=wav, mix_w=fl[0]['mix_w'], start_w=fl[0]['start_w'],
                       start_b=fl[0]['start_b'], h=h)
        else:
            # the same launches; every layer reads its own image of h and the gate values, skip and head rows are kept
            fo = 0
            for b, nf in enumerate(frames):                  # the upsample's operand rows [q][(j, ci)] = mel[q - j][ci]
                for j in range(min(UP_KERNEL // HOP, nf)):
                    sv.xc[fo + j:fo + nf, j * nm:(j + 1) * nm].copy_(mel_cl[b * N:b * N + nf - j])
                fo += nf
            nv.wg_head(rowb, rowr, a_rows, G, B, Rm, wave=wav, mix_w=fl[0]['mix_w'], start_w=fl[0]['start_w'],
                       start_b=fl[0]['start_b'], h=sv.hs[0][0], save=sv.heads[0])
        z_off = c_off = 0
        for k in range(self.n_flows):
            f = fl[k]
            nv.gemm(cnd_r, cond_r, f['cond_w'], bias=f['cond_b'], fast=prec)
            skip_k = skip if sv is None else sv.skip[k]
            for i in range(L):
                last_layer = i == L - 1
                cnd_i = cnd_r[:, 2 * C * i:2 * C * (i + 1)]
                if sv is None:
                    nv.wg_gated(h_r, f['in_w'][i], f['in_b'][i], 2 ** i, cnd_i, acts_r, prec)
                    nv.wg_res_skip(acts_r, f['rs_w'][i], f['rs_b'][i], None if last_layer else h_r, skip_r, i == 0, rowb_r, prec)
                else:
                    h_i = sv.hs[k][i][inner]
                    nv.wg_gated(h_i, f['in_w'][i], f['in_b'][i], 2 ** i, cnd_i, acts_r, prec, gate=sv.gate[k][i][inner])
                    nv.wg_res_skip(acts_r, f['rs_w'][i], f['rs_b'][i], None if last_layer else h_i, skip_k[inner], i == 0,
                                   rowb_r, prec, h_out=None if last_layer else sv.hs[k][i + 1][inner])
            last = k == self.n_flows - 1
            n_in = self.flow_channels[k]
            n_emit = n_in if last else n_in - self.flow_channels[k + 1]
            nxt = None if last else fl[k + 1]
            h_next = None if last else (h if sv is None else sv.hs[k + 1][0])
            nv.wg_head(rowb, rowr, a_rows, G, B, Rm, skip=skip_k, end_w=f['end_w'], end_b=f['end_b'],
                       log_s=log_s[:, c_off:c_off + n_halves[k]], z=z if n_emit else None, z_off=z_off, n_emit=n_emit,
                       mix_w=nxt['mix_w'] if nxt else None, start_w=nxt['start_w'] if nxt else None,
                       start_b=nxt['start_b'] if nxt else None, h=h_next, **({} if sv is None else {'save': sv.heads[k + 1]}))
            z_off += n_emit
            c_off += n_halves[k]
        if sv is not None:
            sv.keep(pk=pk, prec=prec, rowb=rowb, rowr=rowr, offs=offs, frames=frames, rows=rows, cond_g=cond_g, log_s=log_s,
                    B=B, Rm=Rm)
        return z, log_s, rows, sv

    def _split_log_s(self, log_s):
        out, c = [], 0
        for n in self.flow_channels:
            out.append(log_s[:, c:c + n // 2])
            c += n // 2
        return out

    @torch.no_grad()
    def forward(self, forward_input, lengths=None):
        """glow.py's ``forward``: ``forward_input = (spect, audio)`` with (B, n_mel, N) mels and (B, T) audio, T a multiple of
        n_group and at most 256 N (mel frames at or past ceil(T / 256) are not read) -> ``(z, log_s_list, log_det_W_list)``:
        z (B, n_group, T') with T' = T / n_group, the early outputs first; log_s_list[k] (B, n_half_k, T') (views of one
        buffer); log_det_W_list[k] = B T' logdet(W_k), a float32 scalar (nan when det W_k < 0).
        ``lengths``: samples per utterance (ragged: each utterance computed as if alone, z and log_s zero beyond T'_b,
        log_det_W_list[k] = sum_b T'_b logdet(W_k)).
        This entry has no backward pass: the outputs do not require grad, whatever the inputs and the parameters do
        (``training_loss`` is the differentiable one).
        After ``.half()``: bf16 compute, z and log_s float16 (log_det_W_list stays float32: it grows with B T')."""
        spect, audio = forward_input
        z, log_s, rows, _ = self._forward(spect, audio, lengths, "forward")
        logdet = self._packed(z.device)['logdet']
        ld = torch.tensor([sum(rows) * v for v in logdet], dtype=torch.float32, device=z.device)
        if self.half_io:
            z, log_s = z.half(), log_s.half()
        return z, self._split_log_s(log_s), list(ld.unbind(0))

    @torch.no_grad()
    def nll(self, spect, audio, sigma=1.0, lengths=None):
        """(B,) float32: the value ``WaveGlowLoss(sigma)`` gives for each utterance alone (nats per sample), from one
        ``forward`` of the (ragged) batch and the reduction kernel."""
        z, log_s, rows, _ = self._forward(spect, audio, lengths, "nll")
        dev = z.device
        sums = _nll_sums(z, log_s, torch.tensor(rows, dtype=torch.int32, device=dev))
        logdet = self._packed(dev)['logdet']
        # each term rounded to float32 as forward() hands it to the loss, summed in float64
        ld = [float(np.sum(np.float32([r * v for v in logdet]).astype(np.float64))) for r in rows]
        ld = torch.tensor(ld, dtype=torch.float64, device=dev)
        numel = torch.tensor([self.n_group * r for r in rows], dtype=torch.float64, device=dev)
        return ((sums[:, 0] / (2.0 * sigma * sigma) - sums[:, 1] - ld) / numel).float()

    # ---- training: the loss with a backward pass ------------------------------------------------------------------------
    def saved_state_bytes(self, P, n_frames=0):
        """Bytes ``training_loss`` keeps between its forward and its backward for P packed rows: per flow and layer the
        layer's input image h (C floats per row) and the two gate values (2C), per flow skip (C), per flow boundary the
        rows before and after the 1x1 mix (2 n_group), and the upsample's operand rows:
        4 (P (n_flows (3 C L + C) + 2 n_group (n_flows + 1)) + 4 n_mel n_frames)."""
        C, L, G, F = self.n_channels, self.n_layers, self.n_group, self.n_flows
        return 4 * (P * (F * (3 * C * L + C) + 2 * G * (F + 1)) + (UP_KERNEL // HOP) * self.n_mel_channels * n_frames)

    def _loss_value(self, z, log_s, rows, sigma):
        """WaveGlowLoss's arithmetic over the real rows: (sum z^2 / (2 sigma^2) - sum log_s - sum_k sum_b T'_b log det W_k)
        / (n_group sum_b T'_b), the sums in float64 on the reduction kernel."""
        dev = z.device
        sums = _nll_sums(z, log_s, torch.tensor(rows, dtype=torch.int32, device=dev)).sum(0)
        logdet = self._packed(dev)['logdet']
        ld = torch.tensor([sum(rows) * v for v in logdet], dtype=torch.float32, device=dev).double().sum()
        return ((sums[0] / (2.0 * sigma * sigma) - sums[1] - ld) / (self.n_group * sum(rows))).float()

    def training_loss(self, spect, audio, sigma=1.0, lengths=None):
        """The training loss of glow.py, a float32 scalar with a backward pass: ``WaveGlowLoss(sigma)(forward((spect,
        audio)))`` for a full batch (bit for bit: the same launches).  With ``lengths`` (samples per utterance, the rules
        of ``forward``: multiples of n_group, at most 256 N) it is the sum of the per-utterance negative log-likelihoods
        divided by the number of REAL samples sum_b T_b -- the mean over what was scored, not over the padding.

        ``loss.backward()`` gives every parameter of the module that requires grad its float32 gradient, in the
        parameter's own layout, multiplied by the upstream scalar and added into an existing ``.grad``.  The parameters of
        a folded module are the folded weights (``fold_weight_norm``); those of a weight-normed module
        (``apply_weight_norm``) are glow.py's ``weight_g`` / ``weight_v``: the value is that of the folded module built
        from ``fold_weight_norm(state_dict())`` and the gradients of all g / v come from one more launch over the folded
        weights' gradients (csrc/waveglow_wn.hip).  ``spect`` and ``audio`` get no gradient: an input
        that requires grad is refused.  ``precision`` selects the compute of the products in both directions; the
        weights and the gradients are float32 in all three (after ``.half()``: bf16 compute).  Under ``torch.no_grad()``
        (or when no parameter requires grad) the value is the same and nothing is kept.

        Between forward and backward the call keeps ``saved_state_bytes(P, frames)`` bytes in one allocation: 3 C L + C
        floats per packed row and flow (C = 256, L = 8, 12 flows, B = 12 x T = 16000: 26 k rows, 7.7 GB).  Every layer's
        input and gate values are stored rather than recomputed: recomputing a flow's WN would cost a fourth forward per
        step on a part whose memory is not the constraint.  A state that does not fit is refused before anything runs."""
        for name, t in (("mels", spect), ("audio", audio)):
            if torch.is_tensor(t) and t.requires_grad:
                raise ValueError("WaveGlow.training_loss: the %s require grad, but gradients with respect to the inputs are "
                                 "not computed (detach them)" % name)
        params = list(self.parameters())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _TrainingLoss.apply(self, spect, audio, float(sigma), lengths, *params)
        with torch.no_grad():
            z, log_s, rows, _ = self._forward(spect, audio, lengths, "training_loss")
            return self._loss_value(z, log_s, rows, float(sigma))

    def _grad_layout(self):
        """(floats, {parameter name: (offset, shape)}, [(offset, floats) of head call j]) of the flat gradient buffer.  The
        small gradients of one head call are contiguous, in the order the head backward sums them: end of the flow it
        closes (weight, bias), then start (weight, bias) and the 1x1 mix of the flow it opens."""
        C, L, F = self.n_channels, self.n_layers, self.n_flows
        lay, calls, o = {}, [], 0

        def put(name, shape):
            nonlocal o
            lay[name] = (o, tuple(shape))
            o += int(np.prod(shape))

        for j in range(F + 1):
            o0 = o
            if j > 0:
                n_in = self.flow_channels[j - 1]
                put('WN.%d.end.weight' % (j - 1), (n_in, C, 1))
                put('WN.%d.end.bias' % (j - 1), (n_in,))
            if j < F:
                n = self.flow_channels[j]
                put('WN.%d.start.weight' % j, (C, n // 2, 1))
                put('WN.%d.start.bias' % j, (C,))
                put('convinv.%d.conv.weight' % j, (n, n, 1))
            calls.append((o0, o - o0))
        o = -(-o // 4) * 4
        for name, shape in self._folded_shapes():
            if name not in lay:
                put(name, shape)
                o = -(-o // 4) * 4
        return o, lay, calls

    def _backward(self, sv, sigma, upstream):
        """The backward pass over the kept state -> {parameter name: gradient (a view of one flat float32 buffer)}."""
        C, L, G, nm, F, H = self.n_channels, self.n_layers, self.n_group, self.n_mel_channels, self.n_flows, self.halo()
        pk, prec, rowb, rowr, P, B, Rm = sv.pk, sv.prec, sv.rowb, sv.rowr, sv.P, sv.B, sv.Rm
        dev = rowb.device
        fl = pk['flows']
        taps = UP_KERNEL // HOP
        numel = float(G * sum(sv.rows))
        c1, c2 = 1.0 / (sigma * sigma * numel), -1.0 / numel
        total, lay, calls = self._grad_layout()
        gout = torch.empty(total, dtype=torch.float32, device=dev)
        gv = {name: gout[o:o + int(np.prod(shape))].view(shape) for name, (o, shape) in lay.items()}

        # one workspace: [d_cnd | dcat = (dh, d_skip) | acts | dA] zeroed (their halo rows are read as zero), then the rest
        M = P - 2 * H
        sk = [_splitk(2 * C, C, M), _splitk(2 * C * L, G * nm, M)]
        nblk = -(-P // nv.wg_head_bwd_rows())
        npart = max(n for _, n in calls)
        wsN = max(2 * C * L, G * nm)
        sizes = [P * 2 * C * L, P * 2 * C, P * C, P * G,
                 P * G * nm, P * C, max(sk[0] * 2 * C * C, sk[1] * 2 * C * L * G * nm), nblk * npart,
                 2 * C * 3 * C, 2 * C * L * G * nm, HOP * nm * taps * nm, 2 * 2 * 64 * wsN]
        sizes = [-(-n // 4) * 4 for n in sizes]
        bw = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        parts, o = [], 0
        for n in sizes:
            parts.append(bw[o:o + n])
            o += n
        bw[:sum(sizes[:4])].zero_()
        d_cnd = parts[0][:P * 2 * C * L].view(P, 2 * C * L)
        dcat = parts[1][:P * 2 * C].view(P, 2 * C)
        actsb = parts[2][:P * C].view(P, C)
        dA = parts[3][:P * G].view(P, G)
        d_cond_g = parts[4][:P * G * nm].view(P, G * nm)
        d_acts = parts[5][:P * C].view(P, C)
        wpart, hpart = parts[6], parts[7]
        g_in = parts[8][:6 * C * C].view(2 * C, 3 * C)
        g_cond = parts[9][:2 * C * L * G * nm].view(2 * C * L, G * nm)
        g_up = parts[10][:HOP * nm * taps * nm].view(HOP * nm, taps * nm)
        ws64 = parts[11].view(torch.float64)
        inner = slice(H, P - H)
        rowb_r = rowb[inner]
        dh, dskip = dcat[:, :C], dcat[:, C:]
        n_halves = [c // 2 for c in self.flow_channels]
        c_offs = [sum(n_halves[:k]) for k in range(F)]

        def head_bwd(j):
            """Backward of head call j: it closed flow j - 1 and opened flow j."""
            k = j - 1
            n_cur = self.flow_channels[k] if j > 0 else G
            n_out = self.flow_channels[j] if j < F else 0
            kw = {}
            if j > 0:
                kw.update(skip=sv.skip[k], end_w=fl[k]['end_w'], log_s=sv.log_s[:, c_offs[k]:c_offs[k] + n_halves[k]],
                          a_in=sv.heads[k][:, G:], dA=dA, d_skip=dskip)
            if j < F:
                kw.update(dA=dA, dh0=dh, mix_w=fl[j]['mix_w'], start_w=fl[j]['start_w'], a_sv=sv.heads[j][:, G:])
            nb, n = nv.wg_head_bwd(rowb, rowr, G, B, Rm, c1, c2, sv.heads[j][:, :G], hpart, n_emit=n_cur - n_out, **kw)
            o, cnt = calls[j]
            nv.wg_partial_sum(hpart, nb, n, gout[o:o + cnt])
            if j < F:
                gv['convinv.%d.conv.weight' % j].view(n_out, n_out).add_(fl[j]['mix_ldg'])

        head_bwd(F)
        for k in reversed(range(F)):
            f = fl[k]
            pre = 'WN.%d.' % k
            for i in reversed(range(L)):
                last_layer = i == L - 1
                dout = dskip[inner] if last_layer else dcat[inner]                 # gradient of [residual | skip]
                d_pre = d_cnd[inner][:, 2 * C * i:2 * C * (i + 1)]
                nv.gemm(d_acts[inner], dout, f['rs_w'][i], b_kn=True, fast=prec)
                nv.wg_gate_bwd(d_acts[inner], sv.gate[k][i][inner], rowb_r, d_pre, actsb[inner])
                g_rs = gv[pre + 'res_skip_layers.%d.weight' % i]
                _wgrad(g_rs.view(g_rs.shape[0], C), dout, actsb[inner], prec, wpart)
                nv.colsum(dout, ws64, gv[pre + 'res_skip_layers.%d.bias' % i])
                h_i = sv.hs[k][i]
                d = 2 ** i
                for tap in range(3):
                    _wgrad(g_in[:, tap * C:(tap + 1) * C], d_pre, h_i[H + (tap - 1) * d:P - H + (tap - 1) * d], prec, wpart)
                gv[pre + 'in_layers.%d.weight' % i].copy_(g_in.view(2 * C, 3, C).permute(0, 2, 1))
                nv.wg_dgrad(d_pre, f['in_wT'][i], d, dh[inner], last_layer, rowb_r, prec)
            # the cond layer: its bias gradient is every in-layer bias gradient of the flow, side by side
            g_cb = gv[pre + 'cond_layer.bias']
            nv.colsum(d_cnd[inner], ws64, g_cb)
            for i in range(L):
                gv[pre + 'in_layers.%d.bias' % i].copy_(g_cb[2 * C * i:2 * C * (i + 1)])
            _wgrad(g_cond, d_cnd[inner], sv.cond_g[inner], prec, wpart)
            gv[pre + 'cond_layer.weight'].view(2 * C * L, nm, G).copy_(g_cond.view(2 * C * L, G, nm).permute(0, 2, 1))
            nv.gemm(d_cond_g[inner], d_cnd[inner], f['cond_w'], b_kn=True, accumulate=k != F - 1, fast=prec)
            head_bwd(k)

        # the upsample: out[q][p n_mel + co] = sum_(j, ci) mel[q - j][ci] W[ci][co][p + 256 j] + b[co]
        spf = HOP // G
        fo = 0
        for b, nf in enumerate(sv.frames):
            dst = d_cond_g[sv.offs[b]:sv.offs[b] + spf * nf].view(nf, HOP * nm)
            nv.gemm(g_up, dst, sv.xc[fo:fo + nf], a_km=True, b_kn=True, accumulate=b > 0, fast=prec)
            fo += nf
        gv['upsample.weight'].view(nm, nm, taps, HOP).copy_(g_up.view(HOP, nm, taps, nm).permute(3, 1, 2, 0))
        nv.colsum(d_cond_g[inner].reshape(-1, nm), ws64, gv['upsample.bias'])
        gout.mul_(upstream.to(device=dev, dtype=torch.float32))
        if self.weight_norm:
            self._wn_grads(gout, gv)
        return gv


def _nll_sums(z, log_s, rows):
    """(B, 2) float64 {sum z^2, sum log_s} per utterance over its first rows[b] rows (t2amd_wg_nll_f32)."""
    B, _, R = z.shape
    nchunk = -(-R // nv.wg_nll_chunk())
    buf = torch.empty(B * nchunk * 2 + B * 2, dtype=torch.float64, device=z.device)
    out = buf[B * nchunk * 2:].view(B, 2)
    nv.wg_nll(z, log_s, rows, buf[:B * nchunk * 2], out)
    return out


class _SavedState:
    """What ``training_loss`` keeps for its backward pass, in one allocation (``WaveGlow.saved_state_bytes``):
    hs[k][i] [P][C] the input image of layer i of flow k (zero halos), gate[k][i] [P][2C] its tanh | sigmoid values,
    skip[k] [P][C], heads[j] [P][2 n_group] the rows before | after the 1x1 mix of head call j, xc the upsample's operand."""

    def __init__(self, wg, P, n_frames, dev):
        C, L, G, F, nm = wg.n_channels, wg.n_layers, wg.n_group, wg.n_flows, wg.n_mel_channels
        need = wg.saved_state_bytes(P, n_frames)
        if dev.type == 'cuda':
            free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
            if need > free:
                raise nv.NativeError("WaveGlow.training_loss: the state kept for the backward pass needs %.2f GB (%d packed "
                                     "rows x %d flows x (3 C L + C) floats) and %.2f GB are free; use a smaller batch or "
                                     "shorter segments" % (need / 1e9, P, F, free / 1e9))
        sizes = [F * L * P * C, F * L * P * 2 * C, F * P * C, (F + 1) * P * 2 * G, n_frames * (UP_KERNEL // HOP) * nm]
        buf = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        assert buf.numel() * 4 == need
        o = np.cumsum([0] + sizes)
        self.hs = buf[o[0]:o[1]].view(F, L, P, C)
        self.gate = buf[o[1]:o[2]].view(F, L, P, 2 * C)
        self.skip = buf[o[2]:o[3]].view(F, P, C)
        self.heads = buf[o[3]:o[4]].view(F + 1, P, 2 * G)
        self.xc = buf[o[4]:o[5]].view(n_frames, (UP_KERNEL // HOP) * nm)
        self.hs.zero_()
        self.xc.zero_()
        self.P, self.bytes = P, need

    def keep(self, **kw):
        self.__dict__.update(kw)


class _TrainingLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wg, spect, audio, sigma, lengths, *params):
        z, log_s, rows, sv = wg._forward(spect, audio, lengths, "training_loss", save=True)
        ctx.wg, ctx.sv, ctx.sigma = wg, sv, sigma
        ctx.names = [n for n, _ in wg.named_parameters()]
        return wg._loss_value(z, log_s, rows, sigma)

    @staticmethod
    def backward(ctx, upstream):
        if ctx.sv is None:
            raise RuntimeError("WaveGlow.training_loss: backward was already run; the kept state is freed by the first one")
        gv = ctx.wg._backward(ctx.sv, ctx.sigma, upstream)
        ctx.sv = None
        return (None,) * 5 + tuple(gv[n] if need else None for n, need in zip(ctx.names, ctx.needs_input_grad[5:]))


def _one_buffer(tensors):
    """The (B, sum c_k, R) tensor whose consecutive channel slices `tensors` are (what ``WaveGlow.forward`` returns), or
    None."""
    t0 = tensors[0]
    if any(t.dtype != torch.float32 or t.dim() != 3 or t.stride() != t0.stride() or t.shape[0] != t0.shape[0]
           or t.shape[2] != t0.shape[2] or t.device != t0.device for t in tensors):
        return None
    if t0.stride(2) != 1 and t0.shape[2] > 1:
        return None
    ptr_ = t0.data_ptr()
    for t in tensors:
        if t.data_ptr() != ptr_:
            return None
        ptr_ += t.shape[1] * t.stride(1) * 4
    n = sum(t.shape[1] for t in tensors)
    if t0.stride(0) < n * t0.stride(1):
        return None
    return torch.as_strided(t0, (t0.shape[0], n, t0.shape[2]), t0.stride(), t0.storage_offset())


class WaveGlowLoss(nn.Module):
    """glow.py's WaveGlowLoss: ``(sum(z^2) / (2 sigma^2) - sum_k sum(log_s_k) - sum_k log_det_W_k) / z.numel()`` of the
    output of ``WaveGlow.forward``, a float32 scalar.  The two sums run on the reduction kernel (fixed order, float64
    accumulation).  No backward pass: the result does not require grad (``WaveGlow.training_loss`` is the loss that trains)."""

    def __init__(self, sigma=1.0):
        super().__init__()
        self.sigma = sigma

    @torch.no_grad()
    def forward(self, model_output):
        z, log_s_list, log_det_W_list = model_output
        if z.dim() != 3:
            raise ValueError("WaveGlowLoss: expected (B, n_group, T') latents, got %s" % (tuple(z.shape),))
        if not z.is_cuda and not nv.validate_only():
            raise nv.NativeError("WaveGlowLoss: the latents must be on the MI355X; there is no CPU path")
        log_s_list = list(log_s_list)
        for t in log_s_list:
            if t.dim() != 3 or t.shape[0] != z.shape[0] or t.shape[2] != z.shape[2]:
                raise ValueError("WaveGlowLoss: log_s %s beside latents %s" % (tuple(t.shape), tuple(z.shape)))
        z32 = z.float()
        if z32.stride(2) != 1:
            z32 = z32.contiguous()
        log_s = None
        if log_s_list:
            log_s = _one_buffer(log_s_list)
            if log_s is None:
                log_s = torch.cat([t.float() for t in log_s_list], 1)
        rows = torch.full((z.shape[0],), z.shape[2], dtype=torch.int32, device=z.device)
        sums = _nll_sums(z32, log_s, rows).sum(0)
        ld = torch.stack([torch.as_tensor(t, dtype=torch.float32, device=z.device) for t in log_det_W_list]).double().sum()
        sigma = self.sigma
        return ((sums[0] / (2.0 * sigma * sigma) - sums[1] - ld) / z.numel()).float()


class Denoiser(nn.Module):
    """denoiser.py: removes the model bias (the audio of a silent mel) from the magnitude spectrum."""

    def __init__(self, waveglow, filter_length=1024, n_overlap=4, win_length=1024, mode='zeros'):
        super().__init__()
        dev = waveglow.upsample.weight.device
        self.stft = STFT(filter_length=filter_length, hop_length=int(filter_length / n_overlap),
                         win_length=win_length).to(dev)
        if mode == 'zeros':
            mel_input = torch.zeros((1, 80, 88), dtype=torch.float32, device=dev)
        elif mode == 'normal':
            mel_input = torch.randn((1, 80, 88), dtype=torch.float32, device=dev)
        else:
            raise Exception("Mode {} if not supported".format(mode))
        with torch.no_grad():
            bias_audio = waveglow.infer(mel_input, sigma=0.0).float()
            bias_spec, _ = self.stft.transform(bias_audio)
        self.register_buffer('bias_spec', bias_spec[:, :, 0][:, :, None].contiguous())

    def forward(self, audio, strength=0.1):
        audio_spec, audio_angles = self.stft.transform(audio.float())
        nv.wg_denoise(audio_spec, self.bias_spec, strength)
        return self.stft.inverse(audio_spec, audio_angles)


def load_waveglow(src, precision='fp32', weight_norm=False):
    """A WaveGlow from a checkpoint path, a state dict, ``{'model': state dict or module}`` or a module.
    ``weight_norm=True`` keeps ``weight_g`` / ``weight_v`` (a module to go on training); the default folds them."""
    return WaveGlow._from_source(checkpoint_source(src, 'model'), "load_waveglow", precision=precision,
                                 weight_norm=weight_norm)
