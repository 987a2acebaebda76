"""Griffin-Lim vocoder on the MI355X (csrc/vocoder.hip + the GEMMs) against the reference fixture produced by the
unmodified stft.py / audio_processing.py on CPU (tests/golden/make_golden_griffin_lim.py), and its batch contracts."""
import os

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# relative L2 of the signal against the float32 CPU reference.  The reference itself moves by 3.6e-7 / 1.3e-6 / 1.2e-5
# (0 / 1 / 30 iterations) between float32 and float64.  Measured on the MI355X: 7.2e-7 / 5.0e-6 / 1.3e-5 (printed by the
# test); the limits are 3x that.
GL_REL = {0: 2.2e-6, 1: 1.5e-5, 30: 4e-5}


def _golden(name):
    return torch.load(os.path.join(gu.GOLDEN_DIR, name), weights_only=False)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm()).item()


def _sc(stft, mag, x):
    m, _ = stft.transform(x)
    return ((mag.cuda() - m).double().flatten(1).norm(dim=1) / mag.cuda().double().flatten(1).norm(dim=1)).cpu()


def _angles(shape, seed):
    np.random.seed(seed)
    return torch.from_numpy(np.angle(np.exp(2j * np.pi * np.random.rand(*shape))).astype(np.float32))


def test_transform_inverse_forward_match_reference(native_lib):
    from tacotron2_amd.audio import TacotronSTFT
    g = _golden("griffin_lim_demo.pt")
    y = _golden("audio_demo.pt")["y"]
    stft = TacotronSTFT().stft_fn
    mag, phase = stft.transform(y.cuda())
    assert tuple(mag.shape) == tuple(g["mag"].shape) and tuple(phase.shape) == tuple(g["phase"].shape)
    ref = g["mag"]
    assert ((mag.cpu() - ref).abs() <= 1e-4 + 1e-4 * ref.abs()).all()           # test_zz4's magnitude limits
    sel = ref > 1e-3 * ref.max()
    dphi = torch.remainder(phase.cpu() - g["phase"] + torch.pi, 2 * torch.pi) - torch.pi
    print("phase max |diff| where mag > 1e-3 max: %.3e" % dphi[sel].abs().max().item())
    assert dphi[sel].abs().max().item() < 1e-3
    # the existing magnitude path is untouched and agrees
    assert torch.equal(stft.transform_magnitude(y.cuda()), mag)
    inv = stft.inverse(g["mag"].cuda(), g["phase"].cuda())
    assert tuple(inv.shape) == (2, 1, g["inverse"].shape[1])
    r = _rel(inv[:, 0], g["inverse"])
    print("inverse rel L2 %.3e" % r)
    assert r < 1e-5
    rec = stft(y.cuda())                     # forward: transform + inverse reconstructs y (away from the trimmed tail)
    T = rec.shape[-1]
    assert T == (9000 // 256) * 256
    assert _rel(rec[:, 0], y[:, :T]) < 1e-5


def test_griffin_lim_matches_reference_fixture(native_lib):
    from tacotron2_amd.audio import TacotronSTFT, griffin_lim
    g = _golden("griffin_lim_demo.pt")
    stft = TacotronSTFT().stft_fn
    ang = _angles(g["mag"].shape, g["seed"])
    assert abs(ang.double().sum().item() - g["angles_sum"]) < 1e-9
    for n in (0, 1, 30):
        x = griffin_lim(g["mag"].cuda(), stft, n_iters=n, angles=ang)
        assert x.is_cuda and tuple(x.shape) == tuple(g["gl_%d" % n].shape)
        r = _rel(x, g["gl_%d" % n])
        sc = _sc(stft, g["mag"], x)
        print("griffin_lim %2d iterations: rel L2 %.3e, spectral convergence %s (reference %s)"
              % (n, r, sc.tolist(), g["sc_%d" % n].tolist()))
        assert r < GL_REL[n], (n, r)
        assert torch.allclose(sc, g["sc_%d" % n], rtol=5e-5, atol=0), (sc, g["sc_%d" % n])


def test_seeded_draw_equals_explicit_angles(native_lib):
    from tacotron2_amd.audio import TacotronSTFT, griffin_lim
    g = _golden("griffin_lim_demo.pt")
    stft = TacotronSTFT().stft_fn
    np.random.seed(77)
    a = griffin_lim(g["mag"].cuda(), stft, n_iters=3)
    b = griffin_lim(g["mag"].cuda(), stft, n_iters=3, angles=_angles(g["mag"].shape, 77))
    assert torch.equal(a, b)


def _ragged(lengths, seed, F=513):
    gen = torch.Generator().manual_seed(seed)
    mag = torch.zeros(len(lengths), F, max(lengths))
    for b, n in enumerate(lengths):
        mag[b, :, :n] = torch.rand(F, n, generator=gen) * torch.linspace(2.0, 0.01, F)[:, None]
    return mag


def test_ragged_batch_equals_each_utterance_alone(native_lib):
    from tacotron2_amd.audio import TacotronSTFT, griffin_lim
    stft = TacotronSTFT().stft_fn
    lengths = [37, 5, 60, 12]
    mag = _ragged(lengths, 3)
    ang = _angles(mag.shape, 5)
    both = griffin_lim(mag.cuda(), stft, n_iters=4, angles=ang, lengths=lengths)
    assert tuple(both.shape) == (4, 59 * 256)
    for b, n in enumerate(lengths):
        one = griffin_lim(mag[b:b + 1, :, :n].cuda(), stft, n_iters=4, angles=ang[b:b + 1, :, :n].contiguous())
        T = (n - 1) * 256
        assert torch.equal(both[b, :T], one[0]), b
        assert not both[b, T:].any()
    with pytest.raises(RuntimeError, match="reflect"):
        griffin_lim(mag.cuda(), stft, n_iters=1, angles=ang, lengths=[37, 3, 60, 12])


def test_more_than_65535_packed_rows(native_lib):
    from tacotron2_amd.audio import TacotronSTFT, griffin_lim, packed_rows
    stft = TacotronSTFT().stft_fn
    rs = np.random.RandomState(11)
    lengths = [int(v) for v in rs.randint(100, 870, 160)]
    assert packed_rows(lengths) > 65535
    mag = _ragged(lengths, 9)
    ang = _angles(mag.shape, 12)
    out = griffin_lim(mag.cuda(), stft, n_iters=2, angles=ang, lengths=lengths)
    for b in (0, 77, 159):
        n = lengths[b]
        one = griffin_lim(mag[b:b + 1, :, :n].cuda(), stft, n_iters=2, angles=ang[b:b + 1, :, :n].contiguous())
        assert torch.equal(out[b, :(n - 1) * 256], one[0]), b
        assert not out[b, (n - 1) * 256:].any()


def test_bf16x3_within_tolerance_of_fp32(native_lib):
    from tacotron2_amd.audio import TacotronSTFT, griffin_lim
    g = _golden("griffin_lim_demo.pt")
    stft = TacotronSTFT().stft_fn
    ang = _angles(g["mag"].shape, g["seed"])
    a = griffin_lim(g["mag"].cuda(), stft, n_iters=30, angles=ang)
    b = griffin_lim(g["mag"].cuda(), stft, n_iters=30, angles=ang, precision='bf16x3')
    r = _rel(b, a)
    print("bf16x3 vs fp32 after 30 iterations: rel L2 %.3e" % r)
    assert r < 3e-4                      # 7.7e-5 measured
    with pytest.raises(ValueError):
        griffin_lim(g["mag"].cuda(), stft, n_iters=1, angles=ang, precision='bf16')


def test_allocation_count_does_not_grow_with_iterations(native_lib):
    from tacotron2_amd.audio import TacotronSTFT, griffin_lim
    stft = TacotronSTFT().stft_fn
    lengths = [40, 25, 33]
    mag = _ragged(lengths, 1).cuda()
    ang = _angles(mag.shape, 2).cuda()
    griffin_lim(mag, stft, n_iters=1, angles=ang, lengths=lengths)      # tables built

    def count(n):
        torch.cuda.synchronize()
        c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
        griffin_lim(mag, stft, n_iters=n, angles=ang, lengths=lengths)
        torch.cuda.synchronize()
        return torch.cuda.memory_stats()["allocation.all.allocated"] - c0

    assert count(5) == count(50)


def test_mel_to_magnitude_and_mel_path(native_lib):
    from tacotron2_amd.audio import TacotronSTFT
    g = _golden("griffin_lim_demo.pt")
    tac = TacotronSTFT()
    mel = g["mel"]
    mag = tac.mel_to_magnitude(mel.cuda())
    P = np.linalg.pinv(tac.mel_basis.cpu().double().numpy())
    want = np.maximum(np.einsum("fm,bmn->bfn", P, np.exp(mel.double().numpy())), 0.0)
    d = np.abs(mag.cpu().double().numpy() - want)
    assert d.max() <= 1e-5 * np.abs(want).max() + 1e-7, d.max()
    assert torch.equal(tac.mel_to_magnitude(mel.cuda().half()), tac.mel_to_magnitude(mel.cuda().half().float()))
    # zero beyond lengths; the rest unchanged
    part = tac.mel_to_magnitude(mel.cuda(), lengths=[36, 20])
    assert torch.equal(part[0], mag[0]) and torch.equal(part[1, :, :20], mag[1, :, :20]) and not part[1, :, 20:].any()
    x = tac.vocode(mel.cuda(), n_iters=30, angles=_angles(g["mag"].shape, g["seed"]))
    r = _rel(x, g["mel_gl_30"])
    print("mel path 30 iterations: rel L2 %.3e" % r)
    assert r < 1.5e-5                    # 4.3e-6 measured


def test_mel_roundtrip_through_vocode(native_lib):
    from tacotron2_amd.audio import TacotronSTFT
    tac = TacotronSTFT()
    t = torch.arange(22050 * 2, dtype=torch.float64) / 22050.0
    y = 0.3 * torch.sin(2 * np.pi * (150.0 + 400.0 * t) * t)
    for k in (2, 3, 5):
        y = y + 0.1 / k * torch.sin(2 * np.pi * 220.0 * k * t)
    y = y.float()[None]
    mel = tac.mel_spectrogram(y.cuda())
    np.random.seed(1)
    x = tac.vocode(mel, n_iters=30)
    mel2 = tac.mel_spectrogram(torch.clamp(x, -1, 1))
    err = (mel2 - mel).abs().mean().item()
    print("mel -> vocode -> mel: mean |log-mel error| %.4f" % err)
    assert err < 0.6                     # 0.497 measured on the MI355X


def test_vocode_batched_inference_lengths(native_lib):
    from tacotron2_amd.audio import TacotronSTFT
    from tacotron2_amd.model import Tacotron2
    hp = gu.make_hparams(gu.TINY_HP + ",max_decoder_steps=24,gate_threshold=2.0")
    model = Tacotron2(hp)
    model.load_state_dict(gu.build_state_dict(hp, 7))
    model = model.to(DEV).eval()
    text = torch.randint(1, 100, (3, 9), generator=torch.Generator().manual_seed(2)).to(DEV)
    outs = model.inference(text, torch.tensor([9, 7, 4]).to(DEV))
    lens = [int(v) for v in model.last_inference_lengths]
    tac = TacotronSTFT(n_mel_channels=hp.n_mel_channels)
    np.random.seed(0)
    wav = tac.vocode(outs[1].float(), lengths=lens, n_iters=2)
    assert tuple(wav.shape) == (3, (max(lens) - 1) * 256)
    for b, n in enumerate(lens):
        assert not wav[b, (n - 1) * 256:].any()


def test_vocode_cli_writes_wavs(native_lib, tmp_path):
    import subprocess
    import sys
    from scipy.io.wavfile import read
    g = _golden("griffin_lim_demo.pt")
    paths = []
    for b, n in enumerate((36, 21)):
        p = tmp_path / ("utt%d.npy" % b)
        np.save(p, g["mel"][b, :, :n].numpy())
        paths.append(str(p))
    r = subprocess.run([sys.executable, "-m", "tacotron2_amd.vocode"] + paths + ["-o", str(tmp_path / "wav"),
                        "--iters", "3", "--seed", "1"], cwd=gu.ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for b, n in enumerate((36, 21)):
        sr, pcm = read(str(tmp_path / "wav" / ("utt%d.wav" % b)))
        assert sr == 22050 and pcm.dtype == np.int16 and pcm.shape == ((n - 1) * 256,) and np.abs(pcm).max() > 0
