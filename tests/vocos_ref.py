"""Eager torch restatement of the Vocos vocoder (Siuzdak 2023), written from the arithmetic alone (neither the authors' code
nor a checkpoint is at hand): embed, LayerNorm, ConvNeXt blocks (depthwise 7-tap convolution, LayerNorm, Linear, exact GELU,
Linear, gamma, residual), LayerNorm, one linear head giving log-magnitude and phase, mag = min(exp m, 100), and an inverse
STFT (irfft of every frame times the window, overlap-add, division by the overlap-added squared window, 'same' or 'center'
trim).  Plain torch.nn.functional pieces, float64 or float32, CPU or GPU.  The oracle of tests/test_zz16_vocos_gpu.py and
tools/bench_vocos.py.

``make_ref(name, seed)`` draws the weights so that the reference alone exercises what can go wrong (tests/test_vocos_cpu.py
checks it): the head's log-magnitudes have standard deviation 1.5 and a bias that puts 1 % of them, on a fixed random mel,
above log(100), so that between 0.1 % and 5 % of the bins sit at the clamp; its phases are N(0, 2.5^2), far beyond +-pi, and
the output RMS is well above 0.05.  Every weight is a float32 value held in float64, so a float32 module loaded from
``state_dict()`` has exactly the reference's weights."""
import math

import torch
import torch.nn.functional as F

LN_EPS = 1e-6
CLAMP = 100.0

CONFIGS = dict(
    small=dict(n_mel_channels=20, dim=64, intermediate_dim=192, num_layers=2, n_fft=64, hop_length=16, padding='same'),
    odd=dict(n_mel_channels=80, dim=96, intermediate_dim=160, num_layers=3, n_fft=128, hop_length=32, padding='same'),
    center=dict(n_mel_channels=20, dim=64, intermediate_dim=192, num_layers=2, n_fft=64, hop_length=16, padding='center'),
    V=dict(n_mel_channels=80, dim=512, intermediate_dim=1536, num_layers=8, n_fft=1024, hop_length=256, padding='same'),
)


def layer_norm(x, w, b):
    """LayerNorm over the channels of (B, C, N): biased variance, eps 1e-6."""
    return F.layer_norm(x.transpose(1, 2), (x.shape[1],), w, b, LN_EPS).transpose(1, 2)


def convnext_block(x, w, prefix):
    """One block on (B, D, N); w: {name: tensor} with the published names under ``prefix``."""
    D = x.shape[1]
    y = F.conv1d(x, w[prefix + 'dwconv.weight'], w[prefix + 'dwconv.bias'], padding=3, groups=D)
    y = layer_norm(y, w[prefix + 'norm.weight'], w[prefix + 'norm.bias']).transpose(1, 2)
    y = F.linear(y, w[prefix + 'pwconv1.weight'], w[prefix + 'pwconv1.bias'])
    y = y * 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0)))
    y = F.linear(y, w[prefix + 'pwconv2.weight'], w[prefix + 'pwconv2.bias'])
    return x + (w[prefix + 'gamma'] * y).transpose(1, 2)


def overlap_add(frames, hop):
    """(B, L, N) frames -> (B, hop (N - 1) + L): sample j hop + t of the sum gets frames[:, t, j]."""
    B, L, N = frames.shape
    return F.fold(frames, output_size=(1, hop * (N - 1) + L), kernel_size=(1, L), stride=(1, hop))[:, 0, 0, :]


def istft(S, window, hop, padding):
    """Complex (B, F, N) -> (B, samples): 'same' trims (n_fft - hop) / 2 at each end (hop N samples), 'center' n_fft / 2
    (hop (N - 1) samples)."""
    L = window.numel()
    frames = torch.fft.irfft(S, L, dim=1) * window[None, :, None]
    y = overlap_add(frames, hop)
    env = overlap_add((window * window)[None, :, None].expand(1, L, S.shape[2]), hop)
    trim = (L - hop) // 2 if padding == 'same' else L // 2
    end = y.shape[1] - trim
    return y[:, trim:end] / env[:, trim:end]


class VocosRef:
    """weights: {name: tensor} with the published names; config: a dict as in CONFIGS."""

    def __init__(self, config, weights):
        self.config = dict(config)
        self.w = dict(weights)

    def to(self, device=None, dtype=None):
        return VocosRef(self.config, {k: v.to(device=device, dtype=dtype) for k, v in self.w.items()})

    def double(self):
        return self.to(dtype=torch.float64)

    def float(self):
        return self.to(dtype=torch.float32)

    def half(self):
        return self.to(dtype=torch.float16)

    def backbone(self, mel):
        w = self.w
        x = F.conv1d(mel, w['backbone.embed.weight'], w['backbone.embed.bias'], padding=3)
        x = layer_norm(x, w['backbone.norm.weight'], w['backbone.norm.bias'])
        for i in range(self.config['num_layers']):
            x = convnext_block(x, w, 'backbone.convnext.%d.' % i)
        return layer_norm(x, w['backbone.final_layer_norm.weight'], w['backbone.final_layer_norm.bias'])

    def head(self, x):
        """(B, D, N) -> log-magnitude and phase, (B, F, N) each."""
        y = F.linear(x.transpose(1, 2), self.w['head.out.weight'], self.w['head.out.bias']).transpose(1, 2)
        return y.chunk(2, dim=1)

    @torch.no_grad()
    def forward(self, mel):
        m, p = self.head(self.backbone(mel))
        mag = torch.clamp(torch.exp(m), max=CLAMP)
        S = torch.complex(mag * torch.cos(p), mag * torch.sin(p))
        c = self.config
        return istft(S, self.w['head.istft.window'], c['hop_length'], c['padding'])[:, None, :]

    __call__ = forward

    def state_dict(self):
        return {k: v.clone() for k, v in self.w.items()}


def shapes(config):
    """[(name, shape, standard deviation or None for a LayerNorm weight)] of every parameter, in forward order."""
    c = config
    nm, D, I, two_f = c['n_mel_channels'], c['dim'], c['intermediate_dim'], c['n_fft'] + 2

    def norm(name):
        return [(name + '.weight', (D,), None), (name + '.bias', (D,), 0.1)]

    out = [('backbone.embed.weight', (D, nm, 7), (7 * nm) ** -0.5), ('backbone.embed.bias', (D,), 0.1)] + norm('backbone.norm')
    for i in range(c['num_layers']):
        b = 'backbone.convnext.%d.' % i
        out += [(b + 'dwconv.weight', (D, 1, 7), 7 ** -0.5), (b + 'dwconv.bias', (D,), 0.1)] + norm(b + 'norm')
        out += [(b + 'pwconv1.weight', (I, D), D ** -0.5), (b + 'pwconv1.bias', (I,), 0.1),
                (b + 'pwconv2.weight', (D, I), I ** -0.5), (b + 'pwconv2.bias', (D,), 0.1), (b + 'gamma', (D,), 0.5)]
    out += norm('backbone.final_layer_norm')
    out += [('head.out.weight', (two_f, D), D ** -0.5), ('head.out.bias', (two_f,), 0.1)]
    return out


def make_mel(B, N, seed, n_mel=80):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n_mel, N, generator=g) * 0.5 - 4.0


def make_ref(config, seed=0):
    """A float64 VocosRef with seeded weights (see the module text for their scale)."""
    if isinstance(config, str):
        config = CONFIGS[config]
    g = torch.Generator().manual_seed(seed)
    w = {}
    for name, shape, std in shapes(config):
        r = torch.randn(shape, generator=g, dtype=torch.float64)
        w[name] = 1.0 + 0.1 * r if std is None else std * r
    Fb = config['n_fft'] // 2 + 1
    # the final LayerNorm gives unit-variance channels: log-magnitude rows of deviation 1.5, phase rows N(0, 2.5^2)
    w['backbone.final_layer_norm.weight'] = torch.ones_like(w['backbone.final_layer_norm.weight'])
    w['backbone.final_layer_norm.bias'] = torch.zeros_like(w['backbone.final_layer_norm.bias'])
    w['head.out.weight'][:Fb] *= 1.5
    w['head.out.weight'][Fb:] *= 2.5
    w['head.istft.window'] = torch.hann_window(config['n_fft'], periodic=True, dtype=torch.float64)
    ref = VocosRef(config, {k: v.float().double() for k, v in w.items()})
    # shift the log-magnitudes so that 1 % of them, on a fixed random mel, lie above the clamp's log(100)
    with torch.no_grad():
        m, _ = ref.head(ref.backbone(make_mel(1, 48, 12345, config['n_mel_channels']).double()))
    shift = math.log(CLAMP) - torch.quantile(m.flatten(), 0.99).item()
    ref.w['head.out.bias'][:Fb] = (ref.w['head.out.bias'][:Fb] + shift).float().double()
    return ref
