"""WaveGlow's backward pass on the MI355X: ``WaveGlow.training_loss(...).backward()`` against autograd through the float64
restatement (tests/waveglow_fwd_ref.py on waveglow_ref.make_ref(weight_norm=False)) on the same GPU.

Figures per precision: relative error of the loss, worst per-tensor relative L2 of the gradient, relative L2 of all
gradients concatenated.  Measured on the MI355X (B = 2; small: C = 64, L = 4, N = 40; published: C = 256, L = 8, N = 24);
LIMITS below are 3 x the larger of the two geometries (profiles/waveglow_train_pytest_gpu.txt has the run):

                                  loss      worst tensor   all gradients
    float32 restatement  small     7.36e-07  4.06e-07       1.43e-07
                         published 8.27e-07  4.02e-07       1.94e-07
    fp32                 small     1.38e-08  3.20e-07       8.29e-08
                         published 1.22e-08  5.56e-07       1.56e-07
                         ragged    9.30e-09  4.32e-07       8.77e-08   (against the utterances alone: 9.3e-09 6.2e-07 1.1e-07)
    bf16x3               small     1.70e-06  1.65e-05       1.69e-06
                         published 1.95e-06  1.29e-05       2.89e-06
                         ragged    6.66e-07  6.82e-06       1.63e-06   (alone: 1.2e-08 7.2e-06 3.8e-07)
    bf16                 small     2.81e-04  4.75e-03       1.15e-03
                         published 9.62e-04  8.02e-03       1.97e-03
                         ragged    1.26e-04  4.48e-03       1.16e-03   (alone: 6.4e-09 3.4e-03 1.6e-04)
The fp32 loss error is below the resolution of the float32 the loss is returned in, so its limit is 3 x 2^-24.
Training (small geometry, 30 steps, lr 1e-4, FusedAdam against torch.optim.Adam on the float32 restatement): worst relative
distance of the loss curves 1.85e-06 in fp32 (TRACK = 3 x that), 4.66e-04 in bf16; both go from 0.0503 to -0.6955.

The fp32 mode must also stay within 10 x of the float32 restatement's own autograd error on every figure."""
import numpy as np
import pytest
import torch

import waveglow_fwd_ref as fr
import waveglow_ref as wr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LIMITS = {
    'fp32': dict(loss=1.8e-7, worst=1.7e-6, all=4.7e-7),       # loss: 3 x 2^-24, half an ulp of the float32 it is returned in
    'bf16x3': dict(loss=5.9e-6, worst=5.0e-5, all=8.7e-6),
    'bf16': dict(loss=2.9e-3, worst=2.4e-2, all=5.9e-3),
}
RAGGED = dict(LIMITS)              # the ragged batch against the ragged oracle: the same limits
TRACK = 5.6e-6                     # training: worst relative distance of the fp32 loss curve from torch.optim.Adam's
SMALL = dict(C=64, L=4)
PUBLISHED = dict(C=256, L=8)
PRECS = ('fp32', 'bf16x3', 'bf16')


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _models(cfg, seed=0):
    from tacotron2_amd.waveglow import WaveGlow
    ref = wr.make_ref(seed=seed, weight_norm=False, **cfg)
    wg = WaveGlow.from_module(ref).to(DEV).train()
    return ref.double().to(DEV), wg


def _inputs(B, N, seed, T=None):
    g = torch.Generator().manual_seed(seed)
    mel = (torch.randn(B, 80, N, generator=g) * 0.5 - 4.0).to(DEV)
    audio = (0.3 * torch.randn(B, 256 * N if T is None else T, generator=g)).to(DEV)
    return mel, audio


def _oracle(ref, mel, audio, lens=None, sigma=1.0):
    """(loss, {name: gradient}) by autograd through the restatement in ref's dtype; ragged: over the real samples."""
    dt = next(ref.parameters()).dtype
    ref.zero_grad()
    if lens is None:
        out = fr.forward(ref, mel.to(dt), audio.to(dt))
        loss = fr.loss(out, sigma)
        ls_max = max(t.abs().max().item() for t in out[1])
    else:
        z, ls, ld = fr.forward_ragged(ref, mel.to(dt), audio.to(dt), lens)
        loss = fr.loss((z, ls, ld), sigma) * z.numel() / sum(lens)
        ls_max = max(t.abs().max().item() for t in ls)
    loss.backward()
    assert ls_max > 1e-2, "the couplings must not be the identity"
    grads = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    for n, g in grads.items():
        assert g.abs().max().item() > 0, "the oracle's gradient of %s is zero" % n
    return loss.item(), grads


def _figures(loss, grads, want_loss, want):
    names = sorted(want)
    return dict(loss=abs(loss - want_loss) / abs(want_loss), worst=max(_rel(grads[n], want[n]) for n in names),
                all=_rel(torch.cat([grads[n].reshape(-1) for n in names]), torch.cat([want[n].reshape(-1) for n in names])))


def _step(wg, mel, audio, lens=None, sigma=1.0):
    wg.zero_grad(set_to_none=True)
    loss = wg.training_loss(mel, audio, sigma=sigma, lengths=lens)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.requires_grad
    loss.backward()
    return loss.item(), {n: p.grad.detach().clone() for n, p in wg.named_parameters()}


def _check(tag, figs, limits):
    for prec in PRECS:
        print("%s %s: %s" % (tag, prec, " ".join("%s %.3g" % kv for kv in sorted(figs[prec].items()))), flush=True)
    for prec in PRECS:
        for key, lim in limits[prec].items():
            assert lim is not None and figs[prec][key] < lim, (tag, prec, key, figs[prec][key], lim)


@pytest.mark.parametrize("name,cfg,N", [("small", SMALL, 40), ("published", PUBLISHED, 24)])
def test_gradients_match_float64_autograd_per_precision(native_lib, name, cfg, N):
    from tacotron2_amd.waveglow import WaveGlowLoss
    ref, wg = _models(cfg)
    mel, audio = _inputs(2, N, 1)
    want_loss, want = _oracle(ref, mel, audio)
    f32 = _figures(*_oracle(ref.float(), mel, audio), want_loss, want)
    ref.double()
    print("\n%s: loss %.6f; float32 restatement's autograd on the GPU: %s"
          % (name, want_loss, " ".join("%s %.3g" % kv for kv in sorted(f32.items()))), flush=True)
    figs = {}
    for prec in PRECS:
        wg.precision = prec
        loss, grads = _step(wg, mel, audio)
        assert set(grads) == set(want) and all(grads[n].shape == want[n].shape for n in want)
        # the saving forward runs forward's launches: the value is WaveGlowLoss of forward, bit for bit
        assert loss == WaveGlowLoss(1.0)(wg((mel, audio))).item()
        figs[prec] = _figures(loss, grads, want_loss, want)
    _check(name, figs, LIMITS)
    for key in ('worst', 'all'):
        assert figs['fp32'][key] < 10 * f32[key], (name, key, figs['fp32'][key], f32[key])
    assert figs['fp32']['loss'] < 10 * max(f32['loss'], 2.0 ** -24), (name, figs['fp32']['loss'], f32['loss'])


def test_ragged_batch_matches_ragged_oracle_and_the_utterances_alone(native_lib):
    ref, wg = _models(SMALL, seed=8)
    lens = [256 * 30, 256 * 17 - 8 * 11, 256 * 5 + 8]              # whole frames, and two that end inside a frame
    mel, audio = _inputs(3, 30, 2)
    want_loss, want = _oracle(ref, mel, audio, lens)
    figs = {}
    for prec in PRECS:
        wg.precision = prec
        loss, grads = _step(wg, mel, audio, lens)
        figs[prec] = _figures(loss, grads, want_loss, want)
        # the sum of the utterances alone, weighted by their sample counts
        acc, acc_loss = None, 0.0
        for b, t in enumerate(lens):
            nf = -(-t // 256)
            l1, g1 = _step(wg, mel[b:b + 1, :, :nf].contiguous(), audio[b:b + 1, :t].contiguous())
            w = t / sum(lens)
            acc_loss += w * l1
            acc = {n: w * g for n, g in g1.items()} if acc is None else {n: acc[n] + w * g1[n] for n in acc}
        alone = _figures(loss, grads, acc_loss, acc)
        print("ragged %s against the utterances alone: %s" % (prec, " ".join("%s %.3g" % kv for kv in sorted(alone.items()))))
        for key, lim in RAGGED[prec].items():
            assert lim is not None and alone[key] < lim, (prec, key, alone[key], lim)
    _check("ragged", figs, RAGGED)


@pytest.mark.parametrize("prec", PRECS)
def test_two_runs_give_identical_bits(native_lib, prec):
    _, wg = _models(SMALL, seed=3)
    wg.precision = prec
    mel, audio = _inputs(2, 12, 4)
    l1, g1 = _step(wg, mel, audio, [256 * 12, 256 * 7 + 40])
    l2, g2 = _step(wg, mel, audio, [256 * 12, 256 * 7 + 40])
    assert l1 == l2
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


def test_infer_and_forward_are_unchanged_by_a_training_step(native_lib):
    _, wg = _models(SMALL, seed=5)
    mel, audio = _inputs(2, 10, 6)
    noise = [torch.randn(s, device=DEV) for s in wg.noise_shapes(2, 10)]
    a0, f0 = wg.infer(mel, 0.8, z=noise), wg((mel, audio))
    _step(wg, mel, audio)
    a1, f1 = wg.infer(mel, 0.8, z=noise), wg((mel, audio))
    assert torch.equal(a0, a1) and torch.equal(f0[0], f1[0])
    assert all(torch.equal(x, y) for x, y in zip(f0[1], f1[1])) and all(torch.equal(x, y) for x, y in zip(f0[2], f1[2]))
    assert not f1[0].requires_grad


def test_it_trains_and_tracks_torch_adam_on_the_restatement(native_lib):
    from tacotron2_amd.optim import FusedAdam
    steps, lr = 30, 1e-4
    mel, audio = _inputs(2, 16, 9)
    ref, _ = _models(SMALL, seed=11)
    ref = ref.float()
    opt = torch.optim.Adam(ref.parameters(), lr=lr)
    want = []
    for _ in range(steps):
        opt.zero_grad()
        loss = fr.loss(fr.forward(ref, mel, audio))
        loss.backward()
        opt.step()
        want.append(loss.item())
    curves = {}
    for prec in ('fp32', 'bf16'):
        _, wg = _models(SMALL, seed=11)
        wg.precision = prec
        opt = FusedAdam(wg.parameters(), lr=lr)
        got = []
        for _ in range(steps):
            opt.zero_grad()
            loss = wg.training_loss(mel, audio)
            loss.backward()
            opt.step()
            got.append(loss.item())
        curves[prec] = got
        dist = max(abs(a - b) / abs(b) for a, b in zip(got, want))
        print("training %s: first %.6f last %.6f (torch Adam on the restatement: %.6f -> %.6f), worst distance %.3g"
              % (prec, got[0], got[-1], want[0], want[-1], dist), flush=True)
        assert all(np.isfinite(got)) and got[-1] < got[0]
        if prec == 'fp32':
            assert TRACK is not None and dist < TRACK, (dist, TRACK)


def test_allocation_count_does_not_grow_with_layers_or_flows(native_lib):
    """Once .grad exists (autograd clones a parameter's first gradient, one allocation per parameter), a training_loss +
    backward call allocates the same number of blocks whatever the depth."""
    from tacotron2_amd.waveglow import WaveGlow
    counts = []
    for L, flows in ((2, 4), (4, 12)):
        ref = wr.make_ref(C=64, L=L, n_flows=flows, seed=1, weight_norm=False)
        wg = WaveGlow.from_module(ref).to(DEV).train()
        mel, audio = _inputs(2, 6, 3)
        for measured in (False, True):
            wg.zero_grad(set_to_none=False)
            torch.cuda.synchronize()
            c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
            wg.training_loss(mel, audio).backward()
            torch.cuda.synchronize()
            if measured:
                counts.append(torch.cuda.memory_stats()["allocation.all.allocated"] - c0)
    print("allocations per training_loss + backward:", counts)
    assert counts[0] == counts[1], counts


@pytest.mark.parametrize("prec", PRECS)
def test_training_segment_shape_completes(native_lib, prec):
    _, wg = _models(PUBLISHED, seed=2)
    wg.precision = prec
    mel, audio = _inputs(12, 63, 7, T=16000)
    loss, grads = _step(wg, mel, audio)
    assert np.isfinite(loss) and all(torch.isfinite(g).all().item() for g in grads.values())


def test_a_state_that_does_not_fit_is_refused(native_lib):
    from tacotron2_amd import native
    _, wg = _models(PUBLISHED, seed=2)
    free = torch.cuda.mem_get_info(DEV)[0]
    N = 63
    B = int(free * 1.5 / wg.saved_state_bytes(32 * N + 128, N)) + 1
    with pytest.raises(native.NativeError, match="kept for the backward pass needs"):
        wg.training_loss(torch.zeros(B, 80, N, device=DEV), torch.zeros(B, 256 * N, device=DEV))
