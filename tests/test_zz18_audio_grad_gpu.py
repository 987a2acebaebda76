"""The backward pass of the mel front end and the mel L1 loss on the MI355X (TacotronSTFT.mel_spectrogram with a grad_fn,
MelLoss; csrc/audio_bwd.hip) against float64 torch autograd of the restatement (tests/audio_grad_ref.py) on the same GPU, each
new kernel alone against a torch f32 model of itself, and a Vocos fine-tuning loop on top.

The measure is the relative L2 of d_y against float64.  fp32 is held to 10 x the error that the float32 torch autograd of the
same restatement shows against float64 on the same inputs in the same test, which does not depend on the code under test;
bf16x3 to 3 x the figure of the case measured on the MI355X (MEASURED; profiles/audio_grad_pytest_gpu.txt has the run).  The
inputs keep every mel bin 270 x above the clamp and every L1 difference at least 0.1 from its kink
(tests/test_audio_grad_cpu.py asserts both), so no precision puts a value on the other side of either.

Relative L2 of d_y measured (float32 autograd of the restatement beside the two modes):

                          float32 autograd   fp32       bf16x3
    A  sum(out r)         7.22e-07           7.31e-07   6.34e-06
    B  sum(out r)         6.92e-07           6.81e-07   5.48e-06
    C  sum(out r)         5.99e-07           6.04e-07   5.11e-06
    A  MelLoss            6.68e-07           6.75e-07   5.60e-06
    B  MelLoss            6.72e-07           6.97e-07   5.37e-06
    C  MelLoss            5.76e-07           5.77e-07   4.56e-06
    C  MelLoss [12, 1, 6] 5.79e-07           5.87e-07   5.21e-06
    half-silent signal    7.18e-07           8.62e-07   6.61e-06

The largest ratio of an fp32 figure to the float32 autograd's is 1.20 (the half-silent signal).  The loss value differs from
float64 by 1.7e-9 to 1.7e-8 relative (the float32 autograd's by 1.7e-9 to 1.2e-7).
"""
import functools
import json
import os
import sys

import pytest
import torch

import audio_grad_ref as ar
import golden_util as gu
import vocos_grad_ref as gr
import vocos_ref as vr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PRECS = ('fp32', 'bf16x3')
U = 2.0 ** -24
RAGGED = (12, 1, 6)                                  # [n, 1, n // 2] on C
# relative L2 of d_y against float64 with the backward's products in split-bf16, measured on the MI355X
MEASURED = {('A', 'smooth'): 6.34e-6, ('B', 'smooth'): 5.48e-6, ('C', 'smooth'): 5.11e-6,
            ('A', 'l1'): 5.60e-6, ('B', 'l1'): 5.37e-6, ('C', 'l1'): 4.56e-6, ('C', 'ragged'): 5.21e-6}
VOCOS = dict(n_mel_channels=80, dim=32, intermediate_dim=64, num_layers=2, n_fft=1024, hop_length=256, padding='same')
VOCOS_SEED, VOCOS_MEL_SEED = 1, 4                    # the float64 log-magnitudes stay 5.5e-3 from the head's clamp


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def _limit(prec, e32, key):
    if prec == 'fp32':
        return 10.0 * e32
    assert MEASURED[key] is not None, "no measured bf16x3 figure for %s" % (key,)
    return 3.0 * MEASURED[key]


@functools.lru_cache(maxsize=None)
def _stft(name):
    from tacotron2_amd.audio import TacotronSTFT
    return TacotronSTFT(**ar.CASES[name][0]).to(DEV)


@functools.lru_cache(maxsize=None)
def _smooth(name):
    """(y float64 on the GPU, r, float64 gradient, error of the float32 autograd): computed once."""
    geom, B, T = ar.CASES[name]
    y = ar.signal(name).to(DEV)
    r = ar.loss_weights((B, geom['n_mel_channels'], T // geom['hop_length'] + 1), 11).to(DEV)
    g64 = ar.grad_smooth(y, geom, r)
    return y, r, g64, _rel(ar.grad_smooth(y.float(), geom, r), g64)


@functools.lru_cache(maxsize=None)
def _l1(name, lens):
    """(y, target, float64 loss and gradient, errors of the float32 autograd's loss and gradient): computed once."""
    geom = ar.CASES[name][0]
    y = ar.signal(name).to(DEV)
    target = ar.l1_target(ar.logmel(y, geom).cpu(), 12).to(DEV)
    lens = list(lens) if lens else None
    assert ((ar.logmel(y, geom) - target).abs().min().item()) >= ar.MIN_DIFF
    l64, g64 = ar.loss_and_grad_l1(y, geom, target, lens)
    l32, g32 = ar.loss_and_grad_l1(y.float(), geom, target, lens)
    return y, target, l64, g64, abs(l32.item() - l64.item()) / l64.item(), _rel(g32, g64)


# ---- the forward is today's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ar.CASES))
def test_forward_with_grad_is_bit_identical(native_lib, name):
    st = _stft(name)
    y = ar.signal(name).float().to(DEV)
    want = st.mel_spectrogram(y)
    assert not want.requires_grad
    for prec in PRECS:
        got = st.mel_spectrogram(y.clone().requires_grad_(True), precision=prec)
        assert got.grad_fn is not None and got.dtype == torch.float32 and torch.equal(got.detach(), want)
    with torch.no_grad():
        assert st.mel_spectrogram(y.clone().requires_grad_(True)).grad_fn is None


# ---- gradient parity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(ar.CASES))
def test_mel_spectrogram_gradient_parity(native_lib, name, prec):
    st = _stft(name)
    y, r, g64, e32 = _smooth(name)
    x = y.float().requires_grad_(True)
    (st.mel_spectrogram(x, check_range=False, precision=prec) * r.float()).sum().backward()
    assert x.grad.shape == x.shape and x.grad.dtype == torch.float32
    e = _rel(x.grad, g64)
    print("\nFIGURE %s smooth %s: rel L2 %.3e (float32 autograd %.3e)" % (name, prec, e, e32))
    assert e <= _limit(prec, e32, (name, 'smooth')), (name, prec, e, e32)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,lens", [('A', None), ('B', None), ('C', None), ('C', RAGGED)])
def test_mel_loss_value_and_gradient(native_lib, name, lens, prec):
    from tacotron2_amd.audio import MelLoss
    y, target, l64, g64, el32, e32 = _l1(name, lens)
    x = y.float().requires_grad_(True)
    loss = MelLoss(_stft(name))(x, target.float(), lengths=None if lens is None else list(lens), precision=prec)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    el, e = abs(loss.item() - l64.item()) / l64.item(), _rel(x.grad, g64)
    key = (name, 'ragged' if lens else 'l1')
    print("\nFIGURE %s %s %s: loss %.9f rel err %.3e (float32 autograd %.3e), gradient rel L2 %.3e (float32 autograd %.3e)"
          % (name, key[1], prec, loss.item(), el, el32, e, e32))
    assert el <= 10.0 * el32, (name, lens, prec, el, el32)
    assert e <= _limit(prec, e32, key), (name, lens, prec, e, e32)


def test_ragged_batch_is_every_utterance_alone_rescaled(native_lib):
    """The gradient of utterance b inside the ragged batch is its gradient alone times lens_b / sum(lens)."""
    from tacotron2_amd.audio import MelLoss
    y, target, l64, g64, el32, e32 = _l1('C', RAGGED)
    ml = MelLoss(_stft('C'))
    x = y.float().requires_grad_(True)
    ml(x, target.float(), lengths=list(RAGGED)).backward()
    for b, k in enumerate(RAGGED):
        xb = y[b:b + 1].float().requires_grad_(True)
        ml(xb, target[b:b + 1, :, :k].float(), lengths=[k]).backward()
        e = _rel(x.grad[b:b + 1], xb.grad * (k / float(sum(RAGGED))))
        print("\nFIGURE C ragged utterance %d alone: rel L2 %.3e (limit %.3e)" % (b, e, 10.0 * e32))
        assert e <= 10.0 * e32, (b, e, e32)


# ---- clamp and silence -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_silent_frames_give_finite_and_exactly_zero_gradients(native_lib, prec):
    """The second half of the signal is exact zeros: frames 10 .. 16 have mag == 0 everywhere and mel on the clamp.  Sample t
    is covered by frames above (t - 512) / 256 only, so from t = 2816 on every covering frame is silent."""
    geom, T = ar.DEFAULT, 4096
    g = torch.Generator().manual_seed(ar.SIGNAL_SEED)
    y = torch.clamp(0.1 * torch.randn(1, T, generator=g, dtype=torch.float64), -1.0, 1.0)
    y[:, T // 2:] = 0.0
    y = y.to(DEV)
    m64 = ar.mel(y, geom)
    assert (m64[:, :, 10:] == 0).all() and m64[:, :, :10].min().item() >= ar.MIN_MEL
    r = ar.loss_weights((1, 80, T // 256 + 1), 21).to(DEV)
    g64 = ar.grad_smooth(y, geom, r)
    e32 = _rel(ar.grad_smooth(y.float(), geom, r), g64)
    st = _stft('B')
    x = y.float().requires_grad_(True)
    out = st.mel_spectrogram(x, precision=prec)
    silent = out.detach()[:, :, 10:]
    assert (silent == silent[0, 0, 0]).all() and silent[0, 0, 0].item() < -11.5          # log(clip) on every silent bin
    (out * r.float()).sum().backward()
    assert torch.isfinite(x.grad).all()
    assert not x.grad[:, 2816:].any() and not g64[:, 2816:].any()
    e = _rel(x.grad, g64)
    print("\nFIGURE silence %s: rel L2 %.3e (float32 autograd %.3e)" % (prec, e, e32))
    if prec == 'fp32':
        assert e <= 10.0 * e32, (e, e32)
    else:
        assert e <= 3.0 * MEASURED[('B', 'smooth')], e


# ---- determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_two_backward_calls_give_the_same_bits(native_lib, prec):
    from tacotron2_amd.audio import MelLoss
    y, target, *_ = _l1('C', RAGGED)
    ml, grads, losses = MelLoss(_stft('C')), [], []
    for _ in range(2):
        x = y.float().requires_grad_(True)
        loss = ml(x, target.float(), lengths=list(RAGGED), precision=prec)
        loss.backward()
        grads.append(x.grad.clone())
        losses.append(loss.detach().clone())
    assert torch.equal(grads[0], grads[1]) and torch.equal(losses[0], losses[1])
    y, r, *_ = _smooth('A')
    for i in range(2):
        x = y.float().requires_grad_(True)
        (_stft('A').mel_spectrogram(x, precision=prec) * r.float()).sum().backward()
        grads.append(x.grad.clone())
    assert torch.equal(grads[2], grads[3])


# ---- every kernel alone, and what it owns ------------------------------------------------------------------------------------
def _guarded(rows, cols, slack=4):
    """A (rows, cols) view at a row stride of cols + slack inside a buffer of 7.0 with `slack` floats in front and behind."""
    buf = torch.full((rows * (cols + slack) + 2 * slack,), 7.0, device=DEV)
    view = buf[slack:slack + rows * (cols + slack)].view(rows, cols + slack)[:, :cols]
    return buf, view


def _untouched(buf, view):
    mask = torch.ones_like(buf, dtype=torch.bool)
    idx = (view.storage_offset() + torch.arange(view.shape[0], device=DEV)[:, None] * view.stride(0)
           + torch.arange(view.shape[1], device=DEV)[None, :]).reshape(-1)
    mask[idx] = False
    return bool((buf[mask] == 7.0).all())


def test_row_kernels_alone_and_their_ownership(native_lib):
    from tacotron2_amd import native as nv
    g = torch.Generator().manual_seed(31)
    B, n, n_mel, Fb, L, hop = 3, 70, 40, 257, 512, 128          # 70 frames: two 64-frame tiles; 40 mels: 2.5 channel tiles
    T = (n - 1) * hop + 37
    R, Kp = B * n, (2 * Fb + 31) // 32 * 32
    # log-compress backward
    mel = (torch.rand(R, n_mel, generator=g) * 0.1 + 1e-3).to(DEV)
    mel[5, 7], mel[6, 1] = 1e-5, 0.9e-5
    d_out = torch.randn(B, n_mel, n, generator=g).to(DEV)
    buf, d_mel = _guarded(R, n_mel)
    nv.mel_log_bwd(d_out, mel, d_mel, 1e-5)
    want = ar.log_bwd(d_out, mel)
    assert _untouched(buf, d_mel)
    assert (d_mel - want).abs().max().item() <= 4 * U * want.abs().max().item()
    assert d_mel[6, 1] == 0.0 and d_mel[5, 7] != 0.0
    # magnitude backward
    spec = torch.randn(R, 2 * Fb, generator=g).to(DEV)
    spec[3, 9] = spec[3, Fb + 9] = 0.0
    d_mag = torch.randn(R, (Fb + 15) // 16 * 16, generator=g).to(DEV)
    buf, d_spec = _guarded(R, Kp)
    nv.stft_magnitude_bwd(d_mag, spec, d_spec, Fb)
    want = ar.magnitude_bwd(d_mag.cpu(), spec.cpu(), Fb, Kp).to(DEV)
    assert _untouched(buf, d_spec)
    assert (d_spec - want).abs().max().item() <= 8 * U * want.abs().max().item()
    assert d_spec[3, 9] == 0.0 and d_spec[3, Fb + 9] == 0.0 and not d_spec[:, 2 * Fb:].any()
    # overlap-add with the reflect fold: sums of at most 3 positions x L / hop frames
    d_frames = torch.randn(R, L, generator=g).to(DEV)
    buf, d_y = _guarded(B, T, slack=3)
    nv.stft_frames_fold(d_frames, d_y, hop, L // 2)
    want = ar.frames_fold(d_frames.cpu().double(), B, T, L, hop).to(DEV)
    assert _untouched(buf, d_y)
    assert (d_y.double() - want).abs().max().item() <= 4.0 * ((3 * L // hop) ** 0.5 + 4.0) * U * want.abs().max().item()
    # the L1 pair
    out, target = torch.randn(B, n_mel, n, generator=g).to(DEV), torch.randn(B, n_mel, n - 4, generator=g).to(DEV)
    lens = torch.tensor([n - 4, 1, 33], dtype=torch.int32, device=DEV)
    count = n_mel * int(lens.sum())
    slots = nv.mel_l1_slots(B, n_mel, n)
    pbuf = torch.full((slots + 8,), 7.0, device=DEV)
    nv.mel_l1_fwd(out, target, lens, count, pbuf[4:4 + slots])
    assert (pbuf[:4] == 7.0).all() and (pbuf[4 + slots:] == 7.0).all()
    want = ar.l1_loss(out.double(), target.double(), lens.tolist()).item()
    assert abs(pbuf[4:4 + slots].double().sum().item() - want) <= 4 * U * want
    dbuf = torch.full((out.numel() + 8,), 7.0, device=DEV)
    d = dbuf[4:4 + out.numel()].view_as(out)
    gup = torch.tensor([0.7], device=DEV)
    nv.mel_l1_bwd(out, target, lens, gup, count, d)
    assert (dbuf[:4] == 7.0).all() and (dbuf[4 + out.numel():] == 7.0).all()
    assert torch.equal(d, ar.l1_bwd(out, target, lens.tolist(), gup / torch.tensor(float(count), device=DEV), 1.0))


# ---- a Vocos fine-tuning loop ------------------------------------------------------------------------------------------------
def _vocos_case():
    ref = vr.make_ref(VOCOS, VOCOS_SEED).to(DEV)
    mel = vr.make_mel(2, 16, VOCOS_MEL_SEED, 80).to(DEV)
    a64 = gr.audio(ref, mel.double()).detach()
    target = ar.l1_target(ar.logmel(a64[:, 0], ar.DEFAULT)[:, :, :16].cpu(), 13).to(DEV)
    return ref, mel, a64, target


def _train(steps, lr=1e-3):
    from tacotron2_amd.audio import MelLoss
    from tacotron2_amd.optim import FusedAdam
    from tacotron2_amd.vocos import load_vocos
    ref, mel, a64, target = _vocos_case()
    voc = load_vocos(ref.state_dict(), hop_length=256, padding='same').to(DEV).train()
    ml, opt = MelLoss(_stft('B')), FusedAdam(voc.parameters(), lr=lr)
    losses, first = [], None
    for i in range(steps + 1):
        voc.zero_grad(set_to_none=True)
        loss = ml(voc.generate(mel), target.float())
        losses.append(loss.item())
        if i == steps:
            break
        loss.backward()
        if first is None:
            first = {k: p.grad.clone() for k, p in voc.named_parameters()}
        opt.step()
    return losses, first


def test_vocos_fine_tuning_loop(native_lib):
    """20 steps of generate -> MelLoss -> backward -> FusedAdam on one fixed batch (B = 2, 16 frames): the loss falls, two runs
    from the same state give the same losses, and the first step's gradients are float64 autograd's through
    tests/vocos_grad_ref.py composed with the restatement.  Per tensor the limit is the sum of the two fp32 limits: section
    12's, 10 x the float32 autograd's error of the same tensor, here of the composition that this loop differentiates (the
    upstream gradient of the vocoder now carries float32 rounding of its own, which the vocoder's Jacobian passes on to every
    tensor), plus MelLoss's, 10 x the float32 autograd's error of the loss's gradient at the audio."""
    losses, first = _train(20)
    again, _ = _train(20)
    print("\nFIGURE vocos loop: loss %.6f -> %.6f" % (losses[0], losses[-1]))
    assert losses == again
    assert losses[-1] < losses[0]
    ref, mel, a64, target = _vocos_case()
    assert (ar.logmel(a64[:, 0], ar.DEFAULT)[:, :, :16] - target).abs().min().item() >= ar.MIN_DIFF
    assert (gr.log_magnitudes(ref, mel.double()) - torch.log(torch.tensor(vr.CLAMP))).abs().min().item() >= gr.CLAMP_MARGIN
    names = [n for n, _, _ in vr.shapes(ref.config)]

    def composed(dtype):
        leaves = {n: ref.w[n].detach().to(dtype).clone().requires_grad_(True) for n in names}
        leaves['head.istft.window'] = ref.w['head.istft.window'].to(dtype)
        a = gr.audio(vr.VocosRef(ref.config, leaves), mel.to(dtype))
        ar.l1_loss(ar.logmel(a[:, 0], ar.DEFAULT), target).backward()
        return {n: leaves[n].grad for n in names}

    _, da64 = ar.loss_and_grad_l1(a64[:, 0], ar.DEFAULT, target)
    _, da32 = ar.loss_and_grad_l1(a64[:, 0].float(), ar.DEFAULT, target)
    e_loss = _rel(da32, da64)
    g64, g32 = composed(torch.float64), composed(torch.float32)
    bad, worst = [], 0.0
    for n in names:
        e, e32 = _rel(first[n], g64[n]), _rel(g32[n], g64[n])
        lim = 10.0 * e32 + 10.0 * e_loss
        worst = max(worst, e / lim)
        print("FIGURE vocos step 0 %-40s rel L2 %.3e (float32 autograd %.3e) limit %.3e" % (n, e, e32, lim))
        if e > lim:
            bad.append((n, e, lim))
    print("FIGURE vocos step 0 worst ratio to the limit %.3f (loss gradient at the audio: float32 autograd %.3e)" % (worst, e_loss))
    assert not bad, bad


# ---- the shared front end, backward tail and device helpers move no bit -------------------------------------------------------
def _digests(section):
    sys.path.insert(0, gu.GOLDEN_DIR)
    try:
        import make_golden_audio_digests as mk
    finally:
        sys.path.remove(gu.GOLDEN_DIR)
    with open(os.path.join(gu.GOLDEN_DIR, "audio_digests.json")) as fh:
        return mk, json.load(fh)[section]


def test_bits_equal_the_digests_from_before_the_shared_helpers(native_lib):
    """tests/golden/audio_digests.json was written by the commit before audio.py's STFT front ends and spectral backward tails
    became one each and the row kernels took their helpers from csrc/common.h: mel_spectrogram (A, C) and its gradient, MelLoss
    (C, full and ragged), STFT.transform, griffin_lim (2 iterations, ragged) per precision, stft_magnitude_bwd alone with a
    zero tail longer than F; and the two clients of the shared wave sum that no other fixture pins (Vocos' LayerNorm backward,
    WaveGlow's weight-norm fold)."""
    mk, want = _digests("mel")
    got = mk.digests_mel()
    assert set(got) == set(want) and len(want) == 14
    assert got == want, sorted(k for k in want if got[k] != want[k])
    mk, want = _digests("wave_sum_clients")
    got = mk.digests_wave_sum_clients()
    assert set(got) == set(want) and len(want) == 6
    assert got == want, sorted(k for k in want if got[k] != want[k])
