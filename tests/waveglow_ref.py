"""Eager torch restatement of WaveGlow inference (NVIDIA's glow.py and denoiser.py are not in the reference checkout;
this follows the arithmetic spelled out in DESIGN.md section 10).  Structure and parameter names mirror glow.py, with
weight norm on the WN convolutions as NVIDIA trains them.  Runs in float64 or float32 on the CPU or the GPU, and draws
its noise like glow.py: FloatTensor(...).normal_() on the mel's device, first the remaining channels, then one tensor
per early output as it is re-inserted.  The oracle of tests/test_zz11_waveglow_gpu.py and tools/bench_waveglow.py."""
import torch
import torch.nn.functional as F
from torch import nn


class Invertible1x1Conv(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = nn.Conv1d(c, c, kernel_size=1, stride=1, padding=0, bias=False)
        W = torch.linalg.qr(torch.randn(c, c))[0]
        if torch.det(W) < 0:
            W[:, 0] = -W[:, 0]
        self.conv.weight.data = W.view(c, c, 1)

    def inverse(self, z):
        W = self.conv.weight.squeeze()
        W_inv = torch.linalg.inv(W.double().cpu()).to(device=z.device, dtype=z.dtype)
        return F.conv1d(z, W_inv[:, :, None])


class WN(nn.Module):
    def __init__(self, n_in_channels, n_mel_channels, n_layers, n_channels, kernel_size, weight_norm=True):
        super().__init__()
        wn = nn.utils.weight_norm if weight_norm else (lambda m, name='weight': m)
        self.n_layers, self.n_channels = n_layers, n_channels
        self.in_layers = nn.ModuleList()
        self.res_skip_layers = nn.ModuleList()
        self.start = wn(nn.Conv1d(n_in_channels, n_channels, 1), name='weight')
        end = nn.Conv1d(n_channels, 2 * n_in_channels, 1)
        end.weight.data.zero_()
        end.bias.data.zero_()
        self.end = end
        self.cond_layer = wn(nn.Conv1d(n_mel_channels, 2 * n_channels * n_layers, 1), name='weight')
        for i in range(n_layers):
            d = 2 ** i
            self.in_layers.append(wn(nn.Conv1d(n_channels, 2 * n_channels, kernel_size, dilation=d,
                                               padding=(kernel_size * d - d) // 2), name='weight'))
            rs = 2 * n_channels if i < n_layers - 1 else n_channels
            self.res_skip_layers.append(wn(nn.Conv1d(n_channels, rs, 1), name='weight'))

    def forward(self, audio, spect):
        audio = self.start(audio)
        output = torch.zeros_like(audio)
        spect = self.cond_layer(spect)
        C = self.n_channels
        for i in range(self.n_layers):
            pre = self.in_layers[i](audio) + spect[:, 2 * C * i:2 * C * (i + 1)]
            acts = torch.tanh(pre[:, :C]) * torch.sigmoid(pre[:, C:])
            rs = self.res_skip_layers[i](acts)
            if i < self.n_layers - 1:
                audio = audio + rs[:, :C]
                output = output + rs[:, C:]
            else:
                output = output + rs
        return self.end(output)


class WaveGlowRef(nn.Module):
    def __init__(self, n_mel_channels, n_flows, n_group, n_early_every, n_early_size, WN_config, weight_norm=True):
        super().__init__()
        self.config = dict(n_mel_channels=n_mel_channels, n_flows=n_flows, n_group=n_group, n_early_every=n_early_every,
                           n_early_size=n_early_size, WN_config=dict(WN_config), weight_norm=weight_norm)
        self.upsample = nn.ConvTranspose1d(n_mel_channels, n_mel_channels, 1024, stride=256)
        self.n_flows, self.n_group = n_flows, n_group
        self.n_early_every, self.n_early_size = n_early_every, n_early_size
        self.WN = nn.ModuleList()
        self.convinv = nn.ModuleList()
        n_half, n_rem = n_group // 2, n_group
        for k in range(n_flows):
            if k % n_early_every == 0 and k > 0:
                n_half -= n_early_size // 2
                n_rem -= n_early_size
            self.convinv.append(Invertible1x1Conv(n_rem))
            self.WN.append(WN(n_half, n_mel_channels * n_group, weight_norm=weight_norm, **WN_config))
        self.n_remaining_channels = n_rem

    def infer(self, spect, sigma=1.0, z=None):
        """z: the noise tensors (float32) in draw order, or None to draw them like glow.py."""
        spect = self.upsample(spect)
        cut = self.upsample.kernel_size[0] - self.upsample.stride[0]
        spect = spect[:, :, :-cut]
        spect = spect.unfold(2, self.n_group, self.n_group).permute(0, 2, 1, 3)
        spect = spect.contiguous().view(spect.size(0), spect.size(1), -1).permute(0, 2, 1)
        B, R = spect.size(0), spect.size(2)
        zs = list(z) if z is not None else None

        def draw(c):
            t = zs.pop(0) if zs is not None else torch.empty(B, c, R, dtype=torch.float32, device=spect.device).normal_()
            return t.to(device=spect.device, dtype=spect.dtype)

        audio = sigma * draw(self.n_remaining_channels)
        for k in reversed(range(self.n_flows)):
            n_half = audio.size(1) // 2
            a0, a1 = audio[:, :n_half], audio[:, n_half:]
            out = self.WN[k](a0, spect)
            s, b = out[:, n_half:], out[:, :n_half]
            a1 = (a1 - b) / torch.exp(s)
            audio = self.convinv[k].inverse(torch.cat([a0, a1], 1))
            if k % self.n_early_every == 0 and k > 0:
                audio = torch.cat((sigma * draw(self.n_early_size), audio), 1)
        return audio.permute(0, 2, 1).contiguous().view(audio.size(0), -1)


def randomize_end(model, gen=None):
    """NVIDIA's init zeroes `end`, which makes every coupling the identity: give it N(0, 0.02^2) weights and
    N(0, 0.01^2) biases so that the affine inverses do something."""
    with torch.no_grad():
        for wn in model.WN:
            wn.end.weight.normal_(0.0, 0.02, generator=gen)
            wn.end.bias.normal_(0.0, 0.01, generator=gen)
    return model


def make_ref(C=64, L=4, n_flows=12, n_group=8, n_early_every=4, n_early_size=2, n_mel=80, seed=0, weight_norm=True):
    torch.manual_seed(seed)
    m = WaveGlowRef(n_mel, n_flows, n_group, n_early_every, n_early_size,
                    dict(n_layers=L, n_channels=C, kernel_size=3), weight_norm=weight_norm)
    # NVIDIA-like scale: the default conv init is too large for a deep stack of tanh gates at C = 256
    randomize_end(m, torch.Generator().manual_seed(seed + 1))
    return m.eval()


def folded_state_dict(model):
    """state dict with weight norm removed (what WaveGlow.load_state_dict expects, and what glow.py's
    remove_weightnorm leaves)."""
    m = WaveGlowRef(**model.config)
    p = next(model.parameters())
    m = m.to(device=p.device, dtype=p.dtype)
    m.load_state_dict(model.state_dict())
    for wn in m.WN:
        for mod in [wn.start, wn.cond_layer] + list(wn.in_layers) + list(wn.res_skip_layers):
            if hasattr(mod, 'weight_g'):
                nn.utils.remove_weight_norm(mod)
    return m.state_dict()


def coupling_stats(model, spect, sigma, z):
    """max |s| and |b| over all flows of one restatement run (float64): shows the couplings are not the identity."""
    stats = []
    orig = [wn.forward for wn in model.WN]

    def hook(k):
        def f(a, s):
            o = orig[k](a, s)
            h = o.size(1) // 2
            stats.append((o[:, h:].abs().max().item(), o[:, :h].abs().max().item()))
            return o
        return f

    for k, wn in enumerate(model.WN):
        wn.forward = hook(k)
    try:
        model.infer(spect, sigma, z)
    finally:
        for k, wn in enumerate(model.WN):
            wn.forward = orig[k]
    return max(s for s, _ in stats), max(b for _, b in stats)
