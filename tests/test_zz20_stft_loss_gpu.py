"""The multi-resolution STFT loss on the MI355X (audio.MultiResolutionSTFTLoss, csrc/stft_loss.hip) against float64 torch autograd
of the restatement (tests/stft_loss_ref.py) on the same GPU, and ``vocos_train.train_step`` with the loss on top.

The measure of a gradient is the relative L2 of d audio against float64.  fp32 is held to 10 x the error that the float32 torch
autograd of the same restatement shows against float64 on the same inputs in the same test, which does not depend on the code
under test; bf16x3 to 3 x the figure of the case measured on the MI355X (MEASURED; profiles/stft_loss_pytest_gpu.txt has the run).
The loss and its terms are float32 numbers: they are held to 10 x the float32 autograd's own error plus 4 roundings of the stored
value (2^-24 each).  The parity inputs keep every |ln m_x - ln m_y| 30 x above its own float32 error and every power far from the
clamp (tests/test_stft_loss_cpu.py asserts both), so no precision puts a bin on the other side of either kink.

Relative L2 of d audio measured (float32 autograd of the restatement beside the two modes):

                float32 autograd   fp32       bf16x3
    A           7.72e-07           2.75e-06   3.50e-06
    B           9.13e-06           1.01e-05   1.09e-05
    C           3.37e-05           5.12e-05   5.08e-05
    Cr          7.46e-06           9.31e-06   1.00e-05

The largest ratio of an fp32 figure to the float32 autograd's is 3.6 (case A); the float32 autograd's own error is carried by the
log-magnitude term, whose gradient divides by m_x (the spectral-convergence term alone: 2.2e-7 for both).  The loss differs from
float64 by 8e-9 to 8e-8 relative, exactly the float32 autograd's figures; the terms by 3e-8 to 1.5e-7 (float32 autograd 7e-8 to
2.6e-7).
"""
import functools
import json
import os
import sys

import pytest
import torch

import audio_grad_ref as ar
import golden_util as gu
import stft_loss_ref as sr
import vocos_ref as vr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PRECS = ('fp32', 'bf16x3')
U = 2.0 ** -24
# relative L2 of d audio against float64 with the backward's products in split-bf16, measured on the MI355X
MEASURED = {'A': 3.50e-6, 'B': 1.090e-5, 'C': 5.080e-5, 'Cr': 1.001e-5}
VOCOS = dict(n_mel_channels=80, dim=32, intermediate_dim=64, num_layers=2, n_fft=1024, hop_length=256, padding='same')
STEP_RESOLUTIONS = tuple(tuple(4 * v for v in r) for r in sr.RESOLUTIONS)      # the test resolutions at the 4096-sample segment


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


@functools.lru_cache(maxsize=None)
def _module(resolutions=sr.RESOLUTIONS, sc_weight=1.0, mag_weight=1.0, eps=sr.PARITY_EPS):
    from tacotron2_amd.audio import MultiResolutionSTFTLoss
    return MultiResolutionSTFTLoss(resolutions, sc_weight=sc_weight, mag_weight=mag_weight, eps=eps).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name, sc_weight=1.0, mag_weight=1.0):
    """(x, y float64 on the GPU, lens, float64 loss, terms and gradient, the float32 autograd's errors of the three): once."""
    _, _, lens = sr.CASES[name]
    x, y = (s.to(DEV) for s in sr.signals(name))
    lens = list(lens) if lens else None
    l64, t64, g64 = sr.loss_and_grad(x, y, sr.RESOLUTIONS, lens, sc_weight, mag_weight, sr.PARITY_EPS)
    l32, t32, g32 = sr.loss_and_grad(x.float(), y.float(), sr.RESOLUTIONS, lens, sc_weight, mag_weight, sr.PARITY_EPS)
    el32 = abs(l32.item() - l64.item()) / l64.item()
    et32 = ((t32.double() - t64).abs() / t64.abs().clamp(min=1e-300)).max().item() if sc_weight and mag_weight else None
    return x, y, lens, l64, t64, g64, el32, et32, _rel(g32, g64)


def _run(ml, x, y, lens, prec='fp32'):
    a = x.float().requires_grad_(True)
    loss = ml(a, y.float(), lengths=lens, precision=prec)
    loss.backward()
    return loss.detach(), a.grad


# ---- parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_loss_value_and_terms(native_lib, name):
    x, y, lens, l64, t64, g64, el32, et32, e32 = _case(name)
    ml = _module()
    loss = ml(x.float(), y.float(), lengths=lens)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device.type == 'cuda' and loss.grad_fn is None
    terms = ml.last_terms
    assert tuple(terms.shape) == (len(sr.RESOLUTIONS), 2) and terms.dtype == torch.float32 and not terms.requires_grad
    el = abs(loss.item() - l64.item()) / l64.item()
    et = ((terms.double() - t64).abs() / t64.abs()).max().item()
    print("\nFIGURE %s: loss %.9f rel err %.3e (float32 autograd %.3e), terms rel err %.3e (float32 autograd %.3e)"
          % (name, loss.item(), el, el32, et, et32))
    assert el <= 10.0 * el32 + 4 * U, (name, el, el32)
    assert et <= 10.0 * et32 + 4 * U, (name, et, et32)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_gradient_parity(native_lib, name, prec):
    x, y, lens, l64, t64, g64, el32, et32, e32 = _case(name)
    loss, grad = _run(_module(), x, y, lens, prec)
    assert grad.shape == x.shape and grad.dtype == torch.float32
    e = _rel(grad, g64)
    print("\nFIGURE %s %s: gradient rel L2 %.3e (float32 autograd %.3e)" % (name, prec, e, e32))
    if prec == 'fp32':
        assert e <= 10.0 * e32, (name, e, e32)
    else:
        assert MEASURED[name] is not None, "no measured bf16x3 figure for %s" % name
        assert e <= 3.0 * MEASURED[name], (name, e)


@pytest.mark.parametrize("weights", [(1.0, 0.0), (0.0, 1.0)])
def test_each_term_alone(native_lib, weights):
    x, y, lens, l64, t64, g64, el32, _, e32 = _case('Cr', *weights)
    loss, grad = _run(_module(sr.RESOLUTIONS, *weights), x, y, lens)
    el, e = abs(loss.item() - l64.item()) / l64.item(), _rel(grad, g64)
    print("\nFIGURE Cr weights %s: loss rel err %.3e (float32 autograd %.3e), gradient rel L2 %.3e (float32 autograd %.3e)"
          % (weights, el, el32, e, e32))
    assert el <= 10.0 * el32 + 4 * U and e <= 10.0 * e32, (weights, el, el32, e, e32)


def test_single_resolution_is_its_share(native_lib):
    """The loss of resolution r alone is R x its share of the three-resolution loss, sc_r + lm_r: three float32 roundings (the two
    terms as stored, and the single loss)."""
    x, y, lens, *_ = _case('Cr')
    ml = _module()
    ml(x.float(), y.float(), lengths=lens)
    terms = ml.last_terms.double()
    for r, res in enumerate(sr.RESOLUTIONS):
        one = _module((res,))(x.float(), y.float(), lengths=lens).double().item()
        want = (terms[r, 0] + terms[r, 1]).item()
        assert abs(one - want) <= 3 * U * want, (res, one, want)


# ---- many slots ------------------------------------------------------------------------------------------------------------
def test_row_kernels_over_many_slots(native_lib):
    """(B, n, F) = (3, 1700, 1025), ragged: 16 rows per workgroup, 319 slots with a partial last one, so the forward runs many
    workgroups and the finish launch's stride-256 loop runs twice.  Random float32 spectra; the reference is float64 autograd of
    the restatement on those very spectra, so the differences are the kernels' float32 operations alone (the stand-in's
    tolerances, tests/test_stft_loss_cpu.py).  Every slot is poisoned with a value of its own, differently in two runs."""
    from tacotron2_amd import native as nv
    B, n, F, lens = 3, 1700, 1025, (1700, 3, 901)
    eps, scw, magw, up = 1e-7, 0.8, 1.3, 0.7
    g = torch.Generator().manual_seed(23)
    rows, Kp = B * n, (2 * F + 31) // 32 * 32
    sx, sy = (0.1 * torch.randn(rows, 2 * F, generator=g)).to(DEV), (0.1 * torch.randn(rows, 2 * F, generator=g)).to(DEV)
    cnt = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ns = nv.stft_loss_slots(rows, F)
    assert ns == 319 and rows % 16 != 0
    bufs = [torch.arange(3 * ns + 3, dtype=torch.float64, device=DEV) * 1e3 + 7.0,
            -torch.arange(3 * ns + 3, dtype=torch.float64, device=DEV) - 3.0]
    guard = [b[3 * ns:].clone() for b in bufs]
    for buf in bufs:
        nv.stft_loss_fwd(sx, sy, cnt, n, F, eps, buf[:3 * ns])
    assert torch.equal(bufs[0][:3 * ns], bufs[1][:3 * ns])
    assert torch.equal(bufs[0][3 * ns:], guard[0]) and torch.equal(bufs[1][3 * ns:], guard[1])
    loss, terms, coef = (torch.full(s, 7.0, device=DEV) for s in ((1,), (1, 2), (1, 2)))
    nv.stft_loss_finish(bufs[0][:3 * ns], [0, ns], [F * sum(lens)], scw, magw, loss, terms, coef)
    d = torch.full((rows, Kp), 7.0, device=DEV)
    nv.stft_loss_bwd(sx, sy, cnt, coef[0], torch.tensor([up], device=DEV), n, F, eps, d)
    mask = torch.arange(n, device=DEV)[None, :] < cnt[:, None]
    x64 = sx.double().view(B, n, 2 * F).requires_grad_(True)
    y64 = sy.double().view(B, n, 2 * F)
    for s in (0, 1, 200, ns - 1):                                      # a workgroup's slot is the sum over its own 16 rows
        r0, r1 = 16 * s, min(rows, 16 * (s + 1))
        want = sr.sums(sx.double()[r0:r1], sy.double()[r0:r1], mask.reshape(-1)[r0:r1], eps)
        for k in range(3):
            assert abs(bufs[0][3 * s + k].item() - want[k].item()) <= 1e-6 * max(want[k].item(), 1e-30), (s, k)
    want, want_terms = sr.loss_from_spectra([x64], [y64], [mask], scw, magw, eps)
    (want * up).backward()
    A, Bn, Lm = (v.item() for v in sr.sums(x64.detach(), y64, mask, eps))
    got = bufs[0][:3 * ns].view(-1, 3).sum(0)
    assert abs(got[0].item() - A) <= 1e-6 * A and abs(got[1].item() - Bn) <= 1e-6 * Bn and abs(got[2].item() - Lm) <= 1e-5 * Lm
    assert ((terms.double() - want_terms).abs() <= 1e-5 * want_terms.abs()).all()
    assert abs(loss.item() - want.item()) <= 1e-5 * want.item()
    assert abs(coef[0, 0].item() - scw / (A * Bn) ** 0.5) <= 2e-6 * coef[0, 0].item()
    e = (d[:, :2 * F].double() - x64.grad.view(rows, 2 * F)).abs().max().item() / x64.grad.abs().max().item()
    print("\nFIGURE many slots: loss %.9f (float64 %.9f), d_spec max err / max %.3e" % (loss.item(), want.item(), e))
    assert e <= 2e-5
    assert not d[:, 2 * F:].any() and not d[~mask.reshape(-1)].any()


def test_module_over_many_slots(native_lib):
    """One resolution (2048, 16, 1200) on 3 x 22000 ragged samples: 4128 frame rows of 1025 bins, 258 slots, through the module;
    the loss and its terms against float64 as in the cases above."""
    res = ((2048, 16, 1200),)
    g = torch.Generator().manual_seed(29)
    x = torch.clamp(0.1 * torch.randn(3, 22000, generator=g, dtype=torch.float64), -1.0, 1.0).to(DEV)
    y = 0.7 * x + 0.7 * torch.clamp(0.1 * torch.randn(3, 22000, generator=g, dtype=torch.float64), -1.0, 1.0).to(DEV)
    lens = [22000, 5000, 13001]
    from tacotron2_amd import native as nv
    assert nv.stft_loss_slots(3 * (22000 // 16 + 1), 1025) == 258
    with torch.no_grad():
        l64, t64 = sr.loss(x, y, res, lens, 1.0, 1.0, sr.PARITY_EPS)
        l32, t32 = sr.loss(x.float(), y.float(), res, lens, 1.0, 1.0, sr.PARITY_EPS)
    el32 = abs(l32.item() - l64.item()) / l64.item()
    et32 = ((t32.double() - t64).abs() / t64.abs()).max().item()
    ml = _module(res)
    loss = ml(x.float(), y.float(), lengths=lens)
    el = abs(loss.item() - l64.item()) / l64.item()
    et = ((ml.last_terms.double() - t64).abs() / t64.abs()).max().item()
    print("\nFIGURE many slots, module: loss %.9f rel err %.3e (float32 autograd %.3e), terms rel err %.3e (float32 autograd %.3e)"
          % (loss.item(), el, el32, et, et32))
    assert el <= 10.0 * el32 + 4 * U and et <= 10.0 * et32 + 4 * U, (el, el32, et, et32)


# ---- clamp and silence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_half_silent_signals(native_lib, prec):
    """eps = 1e-7; the second half of x and y is exact zeros.  A frame of resolution (L, hop) at index j reads the samples
    [j hop - L/2, j hop + L/2) (mirrored at the ends): every frame that covers a sample t >= T/2 + max L starts at or after T/2, is
    silent in both signals, has p = 0 < eps in every bin and so gradient exactly 0."""
    T, Lmax = 4096, max(r[0] for r in sr.RESOLUTIONS)
    x = torch.clamp(0.1 * torch.randn(1, T, generator=torch.Generator().manual_seed(sr.X_SEED), dtype=torch.float64), -1.0, 1.0)
    y = 0.7 * x + 0.07 * torch.randn(1, T, generator=torch.Generator().manual_seed(sr.Y_SEED), dtype=torch.float64)
    x[:, T // 2:] = 0.0
    y[:, T // 2:] = 0.0
    x, y = x.to(DEV), y.to(DEV)
    l64, _, g64 = sr.loss_and_grad(x, y, sr.RESOLUTIONS, None, 1.0, 1.0, 1e-7)
    loss, grad = _run(_module(eps=1e-7), x, y, None, prec)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    assert grad[:, :T // 2].abs().max() > 0
    assert not grad[:, T // 2 + Lmax:].any() and not g64[:, T // 2 + Lmax:].any()
    print("\nFIGURE half silent %s: loss %.9f (float64 %.9f), gradient rel L2 %.3e" % (prec, loss.item(), l64.item(), _rel(grad, g64)))


def test_equal_signals_give_zero(native_lib):
    """y = x: every A_r is 0, the spectral-convergence term contributes neither value nor gradient, every sign is 0."""
    x, *_ = _case('Cr')
    for prec in PRECS:
        loss, grad = _run(_module(), x, x.clone(), [1500, 333, 800], prec)
        assert loss.item() == 0.0 and torch.isfinite(grad).all() and not grad.any()
    assert not _module().last_terms.any()


# ---- determinism, cropping ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_two_calls_give_the_same_bits(native_lib, prec):
    x, y, lens, *_ = _case('Cr')
    (l0, g0), (l1, g1) = (_run(_module(), x, y, lens, prec) for _ in range(2))
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_longer_target_is_cropped(native_lib):
    x, y, lens, *_ = _case('Cr')
    longer = torch.cat([y, torch.ones(3, 77, dtype=y.dtype, device=DEV)], 1)
    l0, g0 = _run(_module(), x, y, lens)
    l1, g1 = _run(_module(), x, longer, lens)
    l2, g2 = _run(_module(), x.unsqueeze(1), longer.unsqueeze(1), lens)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    assert torch.equal(l0, l2) and torch.equal(g0, g2.view_as(g0)) and g2.shape == (3, 1, 1500)


# ---- the driver's step -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_inputs():
    mel = vr.make_mel(2, 16, 4, 80).to(DEV)
    rec = torch.clamp(0.1 * torch.randn(2, 4096 + 100, generator=torch.Generator().manual_seed(17)), -1.0, 1.0)
    return mel, rec                                                    # the recording on the host and longer, as the loop hands it


def _steps(steps, weight, inline=False, warmup=0):
    """``steps`` optimiser steps from the seeded tiny Vocos -> (the losses, device allocations of every step), after ``warmup``
    steps that are not reported."""
    from tacotron2_amd import vocos_train as vt
    from tacotron2_amd.audio import MelLoss, MultiResolutionSTFTLoss, TacotronSTFT
    from tacotron2_amd.optim import FusedAdam
    from tacotron2_amd.vocos import load_vocos
    mel, rec = _step_inputs()
    voc = load_vocos(vr.make_ref(VOCOS, 1).to(DEV).state_dict(), hop_length=256, padding='same').to(DEV).train()
    ml, opt = MelLoss(TacotronSTFT(**ar.DEFAULT).to(DEV)), FusedAdam(voc.parameters(), lr=1e-3)
    sl = MultiResolutionSTFTLoss(STEP_RESOLUTIONS).to(DEV) if weight > 0 else None
    losses, allocs = [], []
    for i in range(warmup + steps):
        before = torch.cuda.memory_stats(DEV)["allocation.all.allocated"]
        if inline:                                                     # the step as it stood before the second loss existed
            voc.zero_grad()
            loss = ml(voc.generate(mel[:, :, :16].contiguous()), mel[:, :, :16], precision='fp32')
            loss.backward()
            opt.step()
            loss = loss.detach()
        elif sl is None:
            loss = vt.train_step(voc, ml, opt, mel, 16, 16, 'fp32')
        else:
            loss = vt.train_step(voc, ml, opt, mel, 16, 16, 'fp32', sl, weight, rec)
        if i >= warmup:
            allocs.append(torch.cuda.memory_stats(DEV)["allocation.all.allocated"] - before)
            losses.append(loss)
    return [v.item() for v in losses], allocs


def test_driver_step_without_the_weight_is_the_earlier_step(native_lib):
    got, _ = _steps(3, 0.0)
    want, _ = _steps(3, 0.0, inline=True)
    assert got == want and all(v == v for v in got)


def test_driver_steps_with_the_stft_loss(native_lib):
    """20 steps at weight 1: finite, falling, the same bits on a second run."""
    losses, _ = _steps(20, 1.0)
    again, _ = _steps(20, 1.0)
    mel_only, _ = _steps(1, 0.0)
    print("\nFIGURE driver steps: loss %.6f -> %.6f (mel term alone at step 0: %.6f)" % (losses[0], losses[-1], mel_only[0]))
    assert all(v == v and abs(v) != float('inf') for v in losses)
    assert losses == again
    assert losses[-1] < losses[0] and losses[0] > mel_only[0]


def test_a_second_step_allocates_what_the_first_did(native_lib):
    """After one warm-up step (it creates what lives across steps: the per-device tables of the loss's backward, FusedAdam's
    state, the .grad tensors), a step and the identical steps after it make the same number of device allocations."""
    _, allocs = _steps(4, 1.0, warmup=1)
    print("\nFIGURE driver steps: device allocations per step after the warm-up %s" % (allocs,))
    assert allocs[0] > 0 and allocs[1] == allocs[0] and allocs[2] == allocs[0] and allocs[3] == allocs[0], allocs


# ---- the shared front end, backward tail and device helpers move no bit -------------------------------------------------------
def test_bits_equal_the_digests_from_before_the_shared_helpers(native_lib):
    """tests/golden/audio_digests.json was written by the commit before the loss took its STFT front end and its spectral
    backward tail from ``audio.STFT`` and its device helpers from csrc/common.h: value, ``last_terms`` and gradient for the cases
    A and Cr at R = 3 and R = 1 per precision, and stft_loss_bwd alone with a zero tail longer than F."""
    sys.path.insert(0, gu.GOLDEN_DIR)
    try:
        import make_golden_audio_digests as mk
    finally:
        sys.path.remove(gu.GOLDEN_DIR)
    with open(os.path.join(gu.GOLDEN_DIR, "audio_digests.json")) as fh:
        want = json.load(fh)["stft_loss"]
    got = mk.digests_stft_loss()
    assert set(got) == set(want) and len(want) == 9
    assert got == want, sorted(k for k in want if got[k] != want[k])
