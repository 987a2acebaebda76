"""The sample-rate converter on the MI355X (audio.Resample, csrc/resample.hip) against the float64 restatement
(tests/resample_ref.py) and its torch autograd on the same GPU.

The measure is the relative L2 against float64, of the output and of the gradient of sum(y g) for a fixed g.  Both are held to
10 x the error that the float32 torch run of the same restatement shows against float64 on the same input in the same test, which
does not depend on the code under test (the rule of DESIGN.md sections 13 and 14 for fp32 paths).  Every case prints its figures
(``FIGURE`` lines; profiles/resample_pytest_gpu.txt has the run, DESIGN.md section 15 the table)."""
import functools
import subprocess
import sys

import numpy as np
import pytest
import torch

import audio_grad_ref as ar
import golden_util as gu
import resample_ref as rr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MEMORY_RATIO = (1031, 1030)              # 1030 phases of 13 taps: beyond the table's LDS budget
RATIOS = [(3, 2), (2, 3), (7, 5), (320, 147), MEMORY_RATIO]


@functools.lru_cache(maxsize=None)
def _module(pair):
    from tacotron2_amd.audio import Resample
    return Resample(*pair).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(pair, B, T, lens, seed):
    """(x, g float32 on the GPU, float64 y and d_x of the restatement, the float32 torch run's errors of the two): once."""
    x = rr.signal(B, T, seed).to(DEV)
    g = rr.signal(B, rr.output_length(*pair, T), seed + 1).to(DEV)
    lens = list(lens) if lens else None
    out = {}
    for dt in (torch.float64, torch.float32):
        xv = x.to(dt).clone().requires_grad_(True)
        y = rr.resample(xv, *pair, lengths=lens, conv=False)
        (gx,) = torch.autograd.grad(y, xv, g.to(dt))
        out[dt] = (y.detach(), gx)
    y64, gx64 = out[torch.float64]
    return x, g, lens, y64, gx64, rr.rel_l2(out[torch.float32][0], y64), rr.rel_l2(out[torch.float32][1], gx64)


def _run(pair, x, g, lens):
    xv = x.detach().clone().requires_grad_(True)
    out = _module(pair)(xv, lens)
    y = out if lens is None else out[0]
    y.backward(g)
    if lens is not None:
        assert out[1] == [rr.output_length(*pair, n) for n in lens]
    return y.detach(), xv.grad


def _check(pair, B, T, lens, seed):
    x, g, lens, y64, gx64, ef, eb = _case(pair, B, T, lens, seed)
    y, dx = _run(pair, x, g, lens)
    assert y.shape == y64.shape and dx.shape == x.shape and y.dtype == dx.dtype == torch.float32
    rf, rb = rr.rel_l2(y, y64), rr.rel_l2(dx, gx64)
    print("\nFIGURE %s B=%d T=%d lens=%s: forward %.3e (float32 torch %.3e), backward %.3e (float32 torch %.3e)"
          % (pair, B, T, lens, rf, ef, rb, eb))
    assert rf <= 10 * ef and rb <= 10 * eb
    if lens is not None:
        for b, n in enumerate(lens):
            assert not y[b, rr.output_length(*pair, n):].any() and not dx[b, n:].any()
    return y, dx


def _lengths_of(pair):
    o = rr.geometry(*pair)[0]
    return [1, 5, 3 * o, 3 * o + 1, 2125]


@pytest.mark.parametrize("pair", RATIOS)
def test_parity_with_the_restatement(native_lib, pair):
    for T in _lengths_of(pair):
        _check(pair, 1, T, None, 100 + T)


@pytest.mark.parametrize("pair", RATIOS)
def test_ragged_batch_equals_each_utterance_alone(native_lib, pair):
    lens = (1500, 333, 1)
    y, dx = _check(pair, 3, 1500, lens, 7)
    x, g = _case(pair, 3, 1500, lens, 7)[:2]
    for b, n in enumerate(lens):
        m = rr.output_length(*pair, n)
        ya, da = _run(pair, x[b:b + 1, :n].contiguous(), g[b:b + 1, :m].contiguous(), None)
        assert torch.equal(ya[0], y[b, :m]) and torch.equal(da[0], dx[b, :n])


@pytest.mark.parametrize("pair", [(320, 147), (147, 320)])
def test_many_workgroups(native_lib, pair):
    """20 000 samples, each its own value: the output (and the gradient) spans the workgroups' runs many times over; and a ragged
    batch whose utterances end inside a run."""
    _check(pair, 1, 20000, None, 31)
    _check(pair, 3, 5000, (5000, 1237, 2600), 33)


def test_both_table_paths_are_reached(native_lib):
    assert _module((320, 147)).table_paths() == ('lds', 'lds')
    assert _module((147, 320)).table_paths() == ('lds', 'lds')
    assert _module(MEMORY_RATIO).table_paths() == ('memory', 'memory')        # run by the parity and ragged cases above
    _check(MEMORY_RATIO, 1, 4000, None, 35)
    _check((320, 147), 1, 4000, None, 35)


@pytest.mark.parametrize("pair", [(320, 147), MEMORY_RATIO])
def test_two_calls_give_the_same_bits(native_lib, pair):
    x, g = _case(pair, 3, 1500, (1500, 333, 1), 7)[:2]
    a = _run(pair, x, g, [1500, 333, 1])
    b = _run(pair, x, g, [1500, 333, 1])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    full = _run(pair, x, g, [1500] * 3)
    none = _run(pair, x, g, None)
    assert torch.equal(full[0], none[0]) and torch.equal(full[1], none[1])


def test_ranks_identity_and_refusals(native_lib):
    from tacotron2_amd import native
    from tacotron2_amd.audio import Resample, resample
    mod = _module((3, 2))
    x = rr.signal(2, 100, 3).to(DEV)
    assert mod(x[0]).shape == (67,) and mod(x[:, None, :]).shape == (2, 1, 67) and mod.output_length(100) == 67
    assert torch.equal(resample(x, 3, 2), mod(x)) and torch.equal(mod(x[0]), mod(x)[0])
    wide = torch.full((2, 107), 7.0, device=DEV)                      # rows wider than T: a strided view goes in as it is
    wide[:, :100] = x
    assert torch.equal(mod(wide[:, :100]), mod(x))
    same = Resample(16000, 16000)
    assert same(x) is x
    with pytest.raises(native.NativeError, match="no CPU path"):
        mod(x.cpu())
    with pytest.raises(TypeError, match="float32"):
        mod(x.double())
    with pytest.raises(ValueError, match="lengths"):
        mod(x, lengths=[100, 0])
    with pytest.raises(native.NativeError, match="exceeds 4096 samples"):
        Resample(48000, 100)(x)


def _logmel(y, geom):
    """audio_grad_ref.logmel with its strided ``conv1d`` stated as the frames of the reflect-padded signal times the basis
    (``unfold`` and ``matmul``: the same sums, no convolution kernel compiled per shape; tests/test_resample_cpu.py holds the two
    to each other)."""
    L, hop = geom['filter_length'], geom['hop_length']
    fb, mb = ar.tables(geom, y.dtype, y.device)
    B, T = y.shape
    x = torch.nn.functional.pad(y.view(B, 1, 1, T), (L // 2, L // 2, 0, 0), mode='reflect').view(B, -1)
    ft = torch.matmul(x.unfold(-1, L, hop), fb.view(-1, L).t()).transpose(1, 2)
    cutoff = L // 2 + 1
    p = ft[:, :cutoff, :] ** 2 + ft[:, cutoff:, :] ** 2
    pos = p > 0
    mag = torch.where(pos, torch.sqrt(torch.where(pos, p, torch.ones_like(p))), torch.zeros_like(p))
    return torch.log(torch.clamp(torch.matmul(mb, mag), min=ar.CLIP))


def test_composes_with_mel_loss(native_lib):
    """MelLoss of a resampled signal: the loss backpropagates through both autograd functions to finite gradients that match
    float64 autograd of the two restatements composed, to 10 x the float32 autograd's figure."""
    from tacotron2_amd.audio import MelLoss, TacotronSTFT
    pair, geom = (48000, 22050), ar.DEFAULT
    g = torch.Generator().manual_seed(5)
    # 4625 samples become the 2125 of audio_grad_ref's case B: the mel front end's shapes are those of its own parity tests
    x = torch.clamp(0.1 * torch.randn(1, 4625, generator=g, dtype=torch.float64), -1.0, 1.0).to(DEV)
    lens_x = [4000]
    new_len = [rr.output_length(*pair, n) for n in lens_x]
    frames = [n // geom['hop_length'] + 1 for n in new_len]
    lm64 = _logmel(rr.resample(x, *pair, lengths=lens_x, conv=False), geom)
    assert lm64.shape[2] == 2125 // geom['hop_length'] + 1
    for b, n in enumerate(frames):                                    # every counted mel bin is 100 x above the clamp's kink
        assert lm64[b, :, :n].min().item() >= float(np.log(100 * ar.CLIP))
    target = ar.l1_target(lm64.cpu(), 9).to(DEV)
    grads = {}
    for dt in (torch.float64, torch.float32):
        xv = x.to(dt).clone().requires_grad_(True)
        loss = ar.l1_loss(_logmel(rr.resample(xv, *pair, lengths=lens_x, conv=False), geom), target, frames)
        loss.backward()
        grads[dt] = (loss.detach(), xv.grad)
    e32 = rr.rel_l2(grads[torch.float32][1], grads[torch.float64][1])
    stft = TacotronSTFT(**geom).to(DEV)
    xv = x.float().clone().requires_grad_(True)
    y, got_len = _module(pair)(xv, lens_x)
    assert got_len == new_len
    loss = MelLoss(stft)(y, target.float(), lengths=frames)
    loss.backward()
    assert torch.isfinite(xv.grad).all() and xv.grad.abs().max() > 0 and not xv.grad[0, 4000:].any()
    r = rr.rel_l2(xv.grad, grads[torch.float64][1])
    print("\nFIGURE MelLoss o Resample %s: loss %.6f (float64 %.6f), d audio %.3e (float32 autograd %.3e)"
          % (pair, loss.item(), grads[torch.float64][0].item(), r, e32))
    assert r <= 10 * e32


def test_vocode_cli_sampling_rate(native_lib, tmp_path):
    from scipy.io.wavfile import read
    g = torch.load(gu.GOLDEN_DIR + "/griffin_lim_demo.pt", weights_only=False)
    paths = []
    for b, n in enumerate((36, 21)):
        p = tmp_path / ("utt%d.npy" % b)
        np.save(p, g["mel"][b, :, :n].numpy())
        paths.append(str(p))
    r = subprocess.run([sys.executable, "-m", "tacotron2_amd.vocode"] + paths + ["-o", str(tmp_path / "wav"), "--iters", "2",
                        "--seed", "1", "--sampling-rate", "16000"], cwd=gu.ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for b, n in enumerate((36, 21)):
        sr, pcm = read(str(tmp_path / "wav" / ("utt%d.wav" % b)))
        assert sr == 16000 and pcm.dtype == np.int16 and np.abs(pcm).max() > 0
        assert pcm.shape == (rr.output_length(22050, 16000, (n - 1) * 256),)
