"""Eager torch restatement of WaveGlow's forward direction (audio -> latents) and of WaveGlowLoss, on
waveglow_ref.WaveGlowRef.  NVIDIA's glow.py is not in the reference checkout; this follows the arithmetic spelled out
in DESIGN.md section 10 ("Forward direction").  Runs in float64 or float32 on the CPU or the GPU.  The oracle of
tests/test_waveglow_forward_cpu.py, tests/test_zz12_waveglow_forward_gpu.py and tools/bench_waveglow_forward.py."""
import torch
import torch.nn.functional as F


def forward(m, spect, audio):
    """glow.py's WaveGlow.forward((spect, audio)) on the WaveGlowRef `m`: (B, n_mel, N) mels and (B, T) audio, T a
    multiple of n_group and at most 256 N -> (z (B, n_group, T / n_group), log_s_list, log_det_W_list)."""
    G = m.n_group
    s = m.upsample(spect)
    assert s.size(2) >= audio.size(1) and audio.size(1) % G == 0
    s = s[:, :, :audio.size(1)]
    s = s.unfold(2, G, G).permute(0, 2, 1, 3)
    s = s.contiguous().view(s.size(0), s.size(1), -1).permute(0, 2, 1)
    a = audio.unfold(1, G, G).permute(0, 2, 1)
    out, log_s_list, log_det_W_list = [], [], []
    for k in range(m.n_flows):
        if k % m.n_early_every == 0 and k > 0:
            out.append(a[:, :m.n_early_size])
            a = a[:, m.n_early_size:]
        W = m.convinv[k].conv.weight
        log_det_W_list.append(a.size(0) * a.size(2) * torch.logdet(W.squeeze()))
        a = F.conv1d(a, W)
        n_half = a.size(1) // 2
        a0, a1 = a[:, :n_half], a[:, n_half:]
        o = m.WN[k](a0, s)
        log_s, b = o[:, n_half:], o[:, :n_half]
        a1 = torch.exp(log_s) * a1 + b
        log_s_list.append(log_s)
        a = torch.cat([a0, a1], 1)
    out.append(a)
    return torch.cat(out, 1), log_s_list, log_det_W_list


def loss(model_output, sigma=1.0):
    """glow.py's WaveGlowLoss(sigma)(model_output)."""
    z, log_s_list, log_det_W_list = model_output
    log_s_total = sum(t.sum() for t in log_s_list)
    log_det_W_total = sum(log_det_W_list)
    return (torch.sum(z * z) / (2 * sigma * sigma) - log_s_total - log_det_W_total) / z.numel()


def early_outputs(m):
    return [k for k in range(1, m.n_flows) if k % m.n_early_every == 0]


def latents_to_noise(m, z):
    """z of `forward` -> the noise list WaveGlowRef.infer takes: the remaining channels, then the early outputs in reverse."""
    E, n_e = m.n_early_size, len(early_outputs(m))
    return [z[:, E * n_e:]] + [z[:, E * i:E * (i + 1)] for i in reversed(range(n_e))]


def noise_to_latents(m, noise):
    noise = list(noise)
    return torch.cat(noise[:0:-1] + noise[:1], 1)


def forward_ragged(m, spect, audio, lengths):
    """Each utterance alone (its first lengths[b] samples), zero beyond T'_b; log_det_W[k] = sum_b T'_b logdet(W_k)."""
    G = m.n_group
    B, T = audio.shape
    z = torch.zeros(B, G, T // G, dtype=audio.dtype, device=audio.device)
    ls, ld = None, None
    for b, t in enumerate(lengths):
        zb, lsb, ldb = forward(m, spect[b:b + 1], audio[b:b + 1, :t])
        if ls is None:
            ls = [torch.zeros(B, x.size(1), T // G, dtype=audio.dtype, device=audio.device) for x in lsb]
            ld = [torch.zeros_like(x) for x in ldb]
        z[b, :, :t // G] = zb[0]
        for k in range(len(ls)):
            ls[k][b, :, :t // G] = lsb[k][0]
            ld[k] = ld[k] + ldb[k]
    return z, ls, ld
