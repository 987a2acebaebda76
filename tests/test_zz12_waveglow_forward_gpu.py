"""WaveGlow's forward direction on the MI355X (csrc/waveglow_fwd.hip between the products of inference) against the
float64 restatement tests/waveglow_fwd_ref.py: latents, log_s, loss, the round trip through infer, and the batch,
dtype, allocation and CLI contracts.

Measured on the MI355X against the float64 restatement, worst of the small (C = 64, L = 4) and published (C = 256,
L = 8) geometries; the limits below are 3x these:

| quantity                                   | fp32    | bf16x3  | bf16    | float32 restatement on the same GPU |
|--------------------------------------------|---------|---------|---------|-------------------------------------|
| z, relative L2                             | 3.32e-7 | 2.61e-6 | 1.37e-3 | 2.79e-7                             |
| log_s, worst flow's relative L2            | 9.86e-7 | 1.09e-5 | 6.24e-3 | 7.07e-7                             |
| loss (WaveGlowLoss), relative              | 9.92e-8 | 3.18e-6 | 9.50e-4 | 8.02e-7                             |
| round trip infer(forward(audio)) vs audio  | 3.91e-7 | 1.48e-6 | 1.00e-3 | 3.45e-7                             |

.half() (bf16 compute, float16 outputs): z 6.22e-4 on the small geometry.  max |log_s| of the float64 restatement: 0.133
(small), 0.283 (published), so the couplings are not the identity.  The fp32 mode's errors are of the order of the
float32 restatement's (at most 1.4x; the loss less, its sums are accumulated in float64); log_s is a small quantity
(the output of WN itself), hence its larger relative error in the bf16 modes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
import waveglow_fwd_ref as fr
import waveglow_ref as wr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# limit = 3 x the measured error (see the table above): relative L2 of z, worst relative L2 of a flow's log_s, relative
# error of the loss, relative L2 of the round trip infer(forward(audio)) against the audio
LIMITS = {
    'fp32': dict(z=1.0e-6, log_s=3.0e-6, loss=3.0e-7, trip=1.2e-6),
    'bf16x3': dict(z=7.8e-6, log_s=3.3e-5, loss=9.5e-6, trip=4.4e-6),
    'bf16': dict(z=4.1e-3, log_s=1.9e-2, loss=2.9e-3, trip=3.0e-3),
}
HALF_Z = 1.9e-3                # .half(): bf16 compute and float16 outputs (3 x 6.22e-4)
SMALL = dict(C=64, L=4)
PUBLISHED = dict(C=256, L=8)
PRECS = ('fp32', 'bf16x3', 'bf16')


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _models(cfg, seed=0):
    from tacotron2_amd.waveglow import WaveGlow
    ref = wr.make_ref(seed=seed, **cfg)
    wg = WaveGlow.from_module(ref).to(DEV).eval()
    return ref.double().to(DEV), wg


def _inputs(B, N, seed, T=None):
    g = torch.Generator().manual_seed(seed)
    mel = (torch.randn(B, 80, N, generator=g) * 0.5 - 4.0).to(DEV)
    audio = (0.3 * torch.randn(B, 256 * N if T is None else T, generator=g)).to(DEV)
    return mel, audio


def _figures(got, want):
    z, ls, ld = got
    return dict(z=_rel(z, want[0]), log_s=max(_rel(a, b) for a, b in zip(ls, want[1])),
                loss=abs(fr.loss((z.double(), [t.double() for t in ls], [t.double() for t in ld])).item()
                         - fr.loss(want).item()) / abs(fr.loss(want).item()))


@pytest.mark.parametrize("name,cfg,N", [("small", SMALL, 40), ("published", PUBLISHED, 24)])
def test_matches_float64_restatement_per_precision(native_lib, name, cfg, N):
    from tacotron2_amd.waveglow import WaveGlowLoss
    ref, wg = _models(cfg)
    B = 2
    mel, audio = _inputs(B, N, 1)
    with torch.no_grad():
        want = fr.forward(ref, mel.double(), audio.double())
        want_loss = fr.loss(want).item()
        ref32 = ref.float()
        got32 = fr.forward(ref32, mel, audio)
        f32 = _figures(got32, want)
        f32['trip'] = _rel(ref32.infer(mel, 1.0, fr.latents_to_noise(ref32, got32[0])), audio)
        ref.double()
    ls_max = max(t.abs().max().item() for t in want[1])
    print("\n%s: max |log_s| %.3g, loss %.6f; float32 restatement on the GPU: %s"
          % (name, ls_max, want_loss, " ".join("%s %.3g" % kv for kv in sorted(f32.items()))))
    assert ls_max > 1e-2
    figs = {}
    for prec in PRECS:
        wg.precision = prec
        got = wg((mel, audio))
        z, ls, ld = got
        assert z.shape == (B, 8, 32 * N) and z.dtype == torch.float32 and not z.requires_grad
        assert [tuple(t.shape) for t in ls] == [tuple(t.shape) for t in want[1]]
        assert len(ld) == 12 and all(abs(a.item() - b.item()) <= 1e-6 * max(1.0, abs(b.item())) for a, b in zip(ld, want[2]))
        f = _figures(got, want)
        loss = WaveGlowLoss(1.0)(got)
        assert loss.shape == () and loss.dtype == torch.float32
        f['loss'] = abs(loss.item() - want_loss) / abs(want_loss)
        f['trip'] = _rel(wg.infer(mel, 1.0, z=wg.latents_to_noise(z)), audio)
        figs[prec] = f
        print("%s %s: %s" % (name, prec, " ".join("%s %.3g" % kv for kv in sorted(f.items()))))
    for prec in PRECS:
        for key, lim in LIMITS[prec].items():
            assert figs[prec][key] < lim, (name, prec, key, figs[prec][key], lim)
    # the sanity bound on the measurement itself: exact-f32 products are of the float32 restatement's order
    for key in ('z', 'log_s', 'trip'):
        assert figs['fp32'][key] < 10 * f32[key], (name, key, figs['fp32'][key], f32[key])
    assert figs['fp32']['loss'] < 10 * max(f32['loss'], 2.0 ** -24), (name, figs['fp32']['loss'], f32['loss'])


@pytest.mark.parametrize("prec", PRECS)
def test_ragged_equals_alone_bitwise(native_lib, prec):
    from tacotron2_amd.waveglow import WaveGlowLoss
    ref, wg = _models(SMALL, seed=8)
    wg.precision = prec
    lens = [256 * 30, 256 * 17 - 8 * 11, 256 * 5 + 8]              # whole frames, and two that end inside a frame
    N = 30
    mel, audio = _inputs(3, N, 9)
    z, ls, ld = wg((mel, audio), lengths=lens)
    nll = wg.nll(mel, audio, sigma=0.9, lengths=lens)
    assert nll.shape == (3,) and nll.dtype == torch.float32
    logdet = [torch.logdet(c.conv.weight.squeeze().double()).item() for c in ref.convinv]
    for k in range(12):
        want = sum(t // 8 for t in lens) * logdet[k]
        assert abs(ld[k].item() - want) <= 1e-6 * max(1.0, abs(want))
    for b, t in enumerate(lens):
        one = wg((mel[b:b + 1], audio[b:b + 1, :t]))
        assert torch.equal(z[b, :, :t // 8], one[0][0]), (prec, b)
        assert not z[b, :, t // 8:].any()
        for k in range(12):
            assert torch.equal(ls[k][b, :, :t // 8], one[1][k][0]), (prec, b, k)
            assert not ls[k][b, :, t // 8:].any()
        assert torch.equal(nll[b], wg.nll(mel[b:b + 1, :, :-(-t // 256)], audio[b:b + 1, :t], sigma=0.9)[0]), (prec, b)
        # nll is WaveGlowLoss on the utterance alone (float32 results of the same sums)
        loss = WaveGlowLoss(0.9)(one).item()
        assert abs(nll[b].item() - loss) <= 2e-7 * abs(loss), (prec, b, nll[b].item(), loss)
    if prec == 'fp32':
        with torch.no_grad():
            for b in (1, 2):
                t = lens[b]
                want = fr.forward(ref, mel[b:b + 1].double(), audio[b:b + 1, :t].double())
                rel = _rel(z[b:b + 1, :, :t // 8], want[0])
                rel_nll = abs(nll[b].item() - fr.loss(want, 0.9).item()) / abs(fr.loss(want, 0.9).item())
                print("\nutterance %d (%d samples): z %.3g, nll %.3g" % (b, t, rel, rel_nll))
                assert rel < LIMITS['fp32']['z'] and rel_nll < LIMITS['fp32']['loss']


def test_more_than_65535_rows(native_lib):
    ref, wg = _models(SMALL, seed=12)
    N = 2100                                     # 67,200 rows
    mel, audio = _inputs(1, N, 13)
    z, ls, ld = wg((mel, audio))
    with torch.no_grad():
        want = fr.forward(ref, mel.double(), audio.double())
    f = _figures((z, ls, ld), want)
    print("\nN = %d: %s" % (N, " ".join("%s %.3g" % kv for kv in sorted(f.items()))))
    for key in f:
        assert f[key] < LIMITS['fp32'][key], (key, f[key])


def test_training_segment_shape(native_lib):
    """NVIDIA's training shape: 16000 samples, 63 mel frames (the last frame is half used)."""
    ref, wg = _models(SMALL, seed=30)
    mel, audio = _inputs(2, 63, 31, T=16000)
    got = wg((mel, audio))
    assert got[0].shape == (2, 8, 2000)
    with torch.no_grad():
        want = fr.forward(ref, mel.double(), audio.double())
    f = _figures(got, want)
    print("\nT = 16000, N = 63: %s" % " ".join("%s %.3g" % kv for kv in sorted(f.items())))
    for key in f:
        assert f[key] < LIMITS['fp32'][key], (key, f[key])
    # frames at or past ceil(T / 256) are not read
    more = torch.cat([mel, torch.full((2, 80, 3), float('nan'), device=DEV)], 2)
    assert torch.equal(wg((more, audio))[0], got[0])
    with pytest.raises(ValueError, match="at most 256"):
        wg((mel[:, :, :62], audio))
    with pytest.raises(ValueError, match="multiples of n_group"):
        wg((mel, audio[:, :15999]))


def test_allocation_count_does_not_grow_with_layers_or_flows(native_lib):
    from tacotron2_amd.waveglow import WaveGlow
    counts = []
    for L, n_flows in ((2, 4), (6, 4), (2, 12)):
        ref = wr.make_ref(seed=15, C=64, L=L, n_flows=n_flows)
        wg = WaveGlow.from_module(ref).to(DEV).eval()
        mel, audio = _inputs(2, 20, 16)
        wg((mel, audio))                          # weights packed
        torch.cuda.synchronize()
        c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
        wg((mel, audio))
        torch.cuda.synchronize()
        counts.append(torch.cuda.memory_stats()["allocation.all.allocated"] - c0)
    assert counts[0] == counts[1] == counts[2], counts


def test_half_mode(native_lib):
    ref, wg = _models(SMALL, seed=21)
    wg = wg.half()
    assert wg.precision == 'bf16'
    mel, audio = _inputs(1, 20, 22)
    z, ls, ld = wg((mel.half(), audio.half()))
    assert z.dtype == torch.float16 and all(t.dtype == torch.float16 for t in ls)
    assert all(t.dtype == torch.float32 for t in ld)
    with torch.no_grad():
        want = fr.forward(ref, mel.half().double(), audio.half().double())
    rel = _rel(z, want[0])
    print("\n.half(): z relative L2 %.3g" % rel)
    assert rel < HALF_Z
    nll = wg.nll(mel.half(), audio.half())
    assert nll.dtype == torch.float32
    rel_nll = abs(nll[0].item() - fr.loss(want).item()) / abs(fr.loss(want).item())
    print(".half(): nll relative %.3g" % rel_nll)
    assert rel_nll < LIMITS['bf16']['loss']
    assert wg.float().precision == 'fp32'


def test_infer_is_unchanged_by_a_forward_call(native_lib):
    _, wg = _models(SMALL, seed=40)
    mel, audio = _inputs(2, 16, 41)
    torch.manual_seed(7)
    before = wg.infer(mel, 0.666)
    wg((mel, audio))
    wg.nll(mel, audio, lengths=[4096, 2048])
    torch.manual_seed(7)
    after = wg.infer(mel, 0.666)
    assert torch.equal(before, after)


def test_cli_waveglow_score(native_lib, tmp_path):
    from scipy.io import wavfile
    from tacotron2_amd.audio import TacotronSTFT
    from tacotron2_amd.waveglow import WaveGlow
    ref = wr.make_ref(seed=24, **SMALL)
    ckpt = str(tmp_path / "wg.pt")
    torch.save({'model': ref.state_dict()}, ckpt)
    files, pcm = [], []
    for i, n in enumerate([5003, 3001]):
        rs = np.random.RandomState(i)
        x = (0.2 * np.sin(np.arange(n) * 0.05 * (i + 1)) + 0.05 * rs.randn(n)).clip(-1, 1)
        p = str(tmp_path / ("a%d.wav" % i))
        pcm.append((x * 32767).astype(np.int16))
        wavfile.write(p, 22050, pcm[-1])
        files.append(p)
    env = dict(os.environ, PYTHONPATH=gu.ROOT)
    out = subprocess.check_output([sys.executable, "-m", "tacotron2_amd.waveglow_score"] + files +
                                  ["--waveglow", ckpt, "--sigma", "0.9"], env=env, cwd=gu.ROOT, text=True)
    print("\n" + out)
    lines = out.strip().splitlines()
    assert len(lines) == 3 and lines[2].startswith("mean ")
    wg = WaveGlow.from_module(ref).to(DEV).eval()
    stft = TacotronSTFT().to(DEV)
    vals = []
    for i, p in enumerate(files):
        path, n, _, v, _ = lines[i].split()
        assert path == p and int(n) == len(pcm[i]) // 8 * 8
        x = torch.from_numpy(pcm[i].astype(np.float32) / 32768.0)[:int(n)].unsqueeze(0).to(DEV)
        want = wg.nll(stft.mel_spectrogram(x), x, sigma=0.9)[0].item()
        assert np.isfinite(float(v)) and abs(float(v) - want) < 2e-6 * max(1.0, abs(want)), (v, want)
        vals.append((int(n), float(v)))
    mean = sum(n * v for n, v in vals) / sum(n for n, _ in vals)
    assert abs(float(lines[2].split()[1]) - mean) < 2e-6 * max(1.0, abs(mean))
