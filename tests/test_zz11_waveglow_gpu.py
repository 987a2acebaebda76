"""WaveGlow inference on the MI355X (csrc/waveglow.hip, csrc/waveglow_layer.hip and the GEMMs) against the float64
restatement tests/waveglow_ref.py, and its batch, noise, dtype, Denoiser and CLI contracts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
import waveglow_ref as wr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# relative L2 of the waveform against the float64 restatement with the same noise.  Measured on the MI355X (worst of
# the cases below): fp32 3.9e-7, bf16x3 1.9e-6, bf16 9.9e-4; the limits are 3x that.
REL = {'fp32': 1.2e-6, 'bf16x3': 5.7e-6, 'bf16': 3e-3}
SMALL = dict(C=64, L=4)
PUBLISHED = dict(C=256, L=8)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _models(cfg, seed=0):
    from tacotron2_amd.waveglow import WaveGlow
    ref = wr.make_ref(seed=seed, **cfg)
    wg = WaveGlow.from_module(ref).to(DEV).eval()
    return ref.double().to(DEV), wg


def _mel(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 80, N, generator=g) * 0.5 - 4.0).to(DEV)


def _noise(wg, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(DEV) for s in wg.noise_shapes(B, N)]


@pytest.mark.parametrize("name,cfg,N", [("small", SMALL, 40), ("published", PUBLISHED, 24)])
def test_matches_float64_restatement_per_precision(native_lib, name, cfg, N):
    ref, wg = _models(cfg)
    mel, B = _mel(2, N, 1), 2
    z = _noise(wg, B, N, 2)
    want = ref.infer(mel.double(), 0.666, [t.double() for t in z])
    s_max, b_max = wr.coupling_stats(ref, mel.double(), 0.666, [t.double() for t in z])
    print("\n%s: max |s| %.3g, max |b| %.3g" % (name, s_max, b_max))
    assert s_max > 1e-2 and b_max > 1e-2
    for prec in ('fp32', 'bf16x3', 'bf16'):
        wg.precision = prec
        got = wg.infer(mel, sigma=0.666, z=z)
        assert got.shape == (B, 256 * N) and got.dtype == torch.float32
        rel = _rel(got, want)
        print("%s %s: relative L2 %.3g" % (name, prec, rel))
        assert rel < REL[prec], (prec, rel)


@pytest.mark.parametrize("sigma", [0.666, 0.0])
def test_seeded_draws_match_restatement(native_lib, sigma):
    ref, wg = _models(SMALL, seed=3)
    mel = _mel(2, 16, 4)
    torch.manual_seed(11)
    got = wg.infer(mel, sigma=sigma)
    after = torch.cuda.FloatTensor(4).normal_()
    torch.manual_seed(11)
    want = ref.infer(mel.double(), sigma)
    after_ref = torch.cuda.FloatTensor(4).normal_()
    assert torch.equal(after, after_ref), "the generator must advance exactly as the reference's"
    rel = _rel(got, want)
    print("\nseeded sigma=%g: relative L2 %.3g" % (sigma, rel))
    assert rel < REL['fp32']


def test_from_module_equals_load_state_dict(native_lib):
    from tacotron2_amd.waveglow import WaveGlow
    ref = wr.make_ref(seed=5, **SMALL)
    assert any(k.endswith('weight_g') for k in ref.state_dict())
    a = WaveGlow.from_module(ref).to(DEV)
    b = WaveGlow(**{k: v for k, v in ref.config.items() if k != 'weight_norm'})
    b.load_state_dict(wr.folded_state_dict(ref))
    b = b.to(DEV)
    mel = _mel(1, 12, 6)
    z = _noise(a, 1, 12, 7)
    assert torch.equal(a.infer(mel, 0.666, z=z), b.infer(mel, 0.666, z=z))


@pytest.mark.parametrize("prec", ['fp32', 'bf16x3', 'bf16'])
def test_ragged_equals_alone_bitwise(native_lib, prec):
    ref, wg = _models(SMALL, seed=8)
    wg.precision = prec
    lens = [30, 17, 5]
    N = max(lens)
    mel = _mel(3, N, 9)
    z = _noise(wg, 3, N, 10)
    out = wg.infer(mel, 0.666, lengths=lens, z=z)
    for b, n in enumerate(lens):
        alone = wg.infer(mel[b:b + 1, :, :n], 0.666, z=[t[b:b + 1, :, :32 * n] for t in z])
        assert torch.equal(out[b, :256 * n], alone[0]), (prec, b)
        assert not out[b, 256 * n:].any()
    if prec == 'fp32':
        padded = wg.infer(mel, 0.666, z=z)
        rel = _rel(padded, ref.infer(mel.double(), 0.666, [t.double() for t in z]))
        print("\npadded without lengths: relative L2 %.3g" % rel)
        assert rel < REL['fp32']


def test_repeated_lengths_reuse_the_row_map_bitwise(native_lib):
    """The module keeps its last row map (direction, lengths, device) on the device: a call that finds its own map, after
    calls with other lengths and in the other direction, gives the bits of a fresh module's single call."""
    _, wg = _models(SMALL, seed=25)
    G, N, lens = wg.n_group, 40, [1, 7, 40]
    mel = _mel(3, N, 26)
    z = _noise(wg, 3, N, 27)
    wav = (torch.randn(3, 40 * G, generator=torch.Generator().manual_seed(28)) * 0.1).to(DEV)
    samples = [G * n for n in lens]
    first = wg.infer(mel, 0.666, lengths=lens, z=z)
    other = wg.infer(mel, 0.666, lengths=[40, 40, 40], z=z)
    third = wg.infer(mel, 0.666, lengths=lens, z=z)
    assert torch.equal(third, first) and not torch.equal(other, first)
    alone = _models(SMALL, seed=25)[1].infer(mel, 0.666, lengths=lens, z=z)
    assert torch.equal(first, alone) and torch.equal(third, alone)
    n_first = wg.nll(mel, wav, lengths=samples)
    n_other = wg.nll(mel, wav, lengths=[40 * G] * 3)
    n_third = wg.nll(mel, wav, lengths=samples)
    assert torch.equal(n_third, n_first) and not torch.equal(n_other, n_first)
    n_alone = _models(SMALL, seed=25)[1].nll(mel, wav, lengths=samples)
    assert torch.equal(n_first, n_alone) and torch.equal(n_third, n_alone)
    assert torch.equal(wg.infer(mel, 0.666, lengths=lens, z=z), alone)          # back in the first direction


def test_more_than_65535_rows(native_lib):
    ref, wg = _models(SMALL, seed=12)
    N = 2100                                     # 67,200 rows
    mel = _mel(1, N, 13)
    z = _noise(wg, 1, N, 14)
    got = wg.infer(mel, 0.666, z=z)
    rel = _rel(got, ref.infer(mel.double(), 0.666, [t.double() for t in z]))
    print("\nN = %d: relative L2 %.3g" % (N, rel))
    assert rel < REL['fp32']


def test_allocation_count_does_not_grow_with_layers(native_lib):
    counts = []
    for L in (2, 6):
        _, wg = _models(dict(C=64, L=L), seed=15)
        mel = _mel(2, 20, 16)
        z = _noise(wg, 2, 20, 17)
        wg.infer(mel, 0.666, z=z)                 # weights packed
        torch.cuda.synchronize()
        c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
        wg.infer(mel, 0.666, z=z)
        torch.cuda.synchronize()
        counts.append(torch.cuda.memory_stats()["allocation.all.allocated"] - c0)
    assert counts[0] == counts[1], counts


def test_denoiser_equals_stft_composition(native_lib):
    from tacotron2_amd.audio import STFT
    from tacotron2_amd.waveglow import Denoiser
    _, wg = _models(SMALL, seed=18)
    den = Denoiser(wg)
    stft = STFT(1024, 256, 1024).to(DEV)
    bias_audio = wg.infer(torch.zeros(1, 80, 88, device=DEV), sigma=0.0)
    bias_spec = stft.transform(bias_audio)[0][:, :, 0][:, :, None]
    assert torch.equal(den.bias_spec, bias_spec)
    audio = wg.infer(_mel(2, 30, 19), 0.666, z=_noise(wg, 2, 30, 20))
    got = den(audio, strength=0.5)
    mag, ph = stft.transform(audio)
    want = stft.inverse(torch.clamp(mag - bias_spec * 0.5, 0.0), ph)
    assert got.shape == (2, 1, 256 * 30)
    assert torch.equal(got, want)


def test_half_mode(native_lib):
    ref, wg = _models(SMALL, seed=21)
    wg = wg.half()
    assert wg.precision == 'bf16' and wg.upsample.weight.dtype == torch.float32
    for k in wg.convinv:
        k.float()
    assert wg.precision == 'bf16'
    mel = _mel(1, 20, 22)
    z = _noise(wg, 1, 20, 23)
    out = wg.infer(mel.half(), 0.666, z=z)
    assert out.dtype == torch.float16
    rel = _rel(out.float(), ref.infer(mel.half().double(), 0.666, [t.double() for t in z]))
    print("\n.half(): relative L2 %.3g" % rel)
    assert rel < REL['bf16']
    assert wg.float().precision == 'fp32'


def test_cli_waveglow_and_denoise(native_lib, tmp_path):
    from scipy.io import wavfile
    ref = wr.make_ref(seed=24, **SMALL)
    ckpt = str(tmp_path / "wg.pt")
    torch.save({'model': ref.state_dict()}, ckpt)
    lens = [12, 7]
    files = []
    for i, n in enumerate(lens):
        p = str(tmp_path / ("m%d.npy" % i))
        np.save(p, (np.random.RandomState(i).randn(80, n) * 0.5 - 4.0).astype(np.float32))
        files.append(p)
    out = str(tmp_path / "wav")
    env = dict(os.environ, PYTHONPATH=gu.ROOT)
    subprocess.check_call([sys.executable, "-m", "tacotron2_amd.vocode"] + files +
                          ["-o", out, "--waveglow", ckpt, "--denoise", "0.01", "--seed", "1"], env=env, cwd=gu.ROOT)
    for i, n in enumerate(lens):
        sr, x = wavfile.read(os.path.join(out, "m%d.wav" % i))
        assert x.dtype == np.int16 and x.shape == (256 * n,)
