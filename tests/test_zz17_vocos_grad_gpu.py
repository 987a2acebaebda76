"""The backward pass of the Vocos vocoder on the MI355X (Vocos.generate; csrc/vocos_bwd.hip) against float64 torch autograd of
the restatement (tests/vocos_grad_ref.py) on the same GPU, each new kernel alone against torch f32, and the batch, determinism,
weight-update and allocation contracts.

The loss is L = sum(audio * r), r a seeded randn / sqrt(T): linear, so a test sees the Jacobian transpose and nothing else.
The measure is the relative L2 of every gradient tensor (every parameter and the mels; none skipped, no element masked)
against float64.  fp32 is held, per tensor, to 10 x the error that the float32 torch autograd of the same restatement shows
against float64 in the same test, which does not depend on the code under test.  bf16x3 and bf16 are held, per tensor, to 3 x
the worst tensor's figure of the case measured on the MI355X (MEASURED, profiles/vocos_grad_pytest_gpu.txt has the run).
A bin on the other side of the clamp than in float64 is a discontinuity of the model, not an error of a kernel (one such
bin moves most gradients by 1e-1): tests/vocos_grad_ref.py chooses the seeds, tests/test_vocos_grad_cpu.py asserts the margin
the float64 log-magnitudes keep from log(100), and the test below asserts for every case and precision that the forward it
differentiates has every bin on the float64 side.

Worst per-tensor relative L2 measured (B x frames; the float32 autograd's worst tensor beside the three modes' worst):

                         float32 autograd   fp32       bf16x3     bf16
    small   2 x 40       9.37e-07           1.07e-06   3.44e-05   1.14e-02
    odd     2 x 40       1.99e-06           3.35e-06   4.00e-05   1.47e-02
    center  2 x 40       7.48e-07           9.47e-07   2.57e-05   8.74e-03
    V       1 x 64       4.84e-06           5.03e-06   4.88e-05   1.65e-02
    small   [3, 1, 140]  5.66e-06           5.23e-06   1.29e-04   2.94e-02

The largest ratio of an fp32 tensor to the float32 autograd's error of the same tensor is 2.43 (odd, convnext.0.norm.weight).
In the ragged case the float32 autograd's own error is 6 times that of small 2 x 40, and the three modes' follow it (worst
tensor in all of them: convnext.0.dwconv.bias and its neighbours, sums over 144 rows of terms that cancel).
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import vocos_grad_ref as gr
import vocos_ref as vr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PRECS = ('fp32', 'bf16x3', 'bf16')
LENS = [3, 1, 140]                                   # more than one 128-row tile, a one-frame utterance
DI = [(64, 192), (96, 160), (512, 1536)]
U = 2.0 ** -24
# worst per-tensor relative L2 against float64 of the case, measured on the MI355X
MEASURED = {
    ('small', (40, 40)): {'bf16x3': 3.44e-5, 'bf16': 1.14e-2},
    ('odd', (40, 40)): {'bf16x3': 4.00e-5, 'bf16': 1.47e-2},
    ('center', (40, 40)): {'bf16x3': 2.57e-5, 'bf16': 8.74e-3},
    ('V', (64,)): {'bf16x3': 4.88e-5, 'bf16': 1.65e-2},
    ('small', (3, 1, 140)): {'bf16x3': 1.29e-4, 'bf16': 2.94e-2},
}


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def kernel_rel(K):
    """As tests/test_zz16_vocos_gpu.py: one kernel alone against torch f32, both sides rounding a sum of K terms in different
    orders, u sqrt K for the two; four times that plus 4 u a side for the element-wise arithmetic."""
    return 4.0 * (K ** 0.5 + 4.0) * U


@functools.lru_cache(maxsize=None)
def _ref(name, seed=gr.WEIGHT_SEED):
    return vr.make_ref(name, seed)


def _module(name, seed=gr.WEIGHT_SEED):
    from tacotron2_amd.vocos import load_vocos
    ref = _ref(name, seed)
    c = ref.config
    return load_vocos(ref.state_dict(), hop_length=c['hop_length'], padding=c['padding']).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name, lens, seed):
    """(ref on the GPU, mel, lengths or None, r, float64 gradients, per-tensor error of the float32 autograd): computed once."""
    ref = _ref(name).to(DEV)
    c = ref.config
    N = max(lens)
    mel = vr.make_mel(len(lens), N, seed, c['n_mel_channels']).to(DEV)
    lengths = list(lens) if len(set(lens)) > 1 else None
    T = c['hop_length'] * N if c['padding'] == 'same' else c['hop_length'] * (N - 1)
    r = gr.loss_weights((len(lens), 1, T), seed + 100).to(DEV)
    g64 = gr.grads(ref, mel.double(), r, lengths)
    g32 = gr.grads(ref.float(), mel, r, lengths)
    e32 = {k: _rel(g32[k], g64[k]) for k in g64}
    return ref, mel, lengths, r, g64, e32


def _grads(voc, mel, lengths, r, want_mel=True, m64=None):
    """The module's gradients; with ``m64`` (the float64 log-magnitudes per utterance, (F, n) each) also the number of bins
    that the forward being differentiated has on the other side of the clamp."""
    voc.zero_grad(set_to_none=True)
    x = mel.clone().requires_grad_(want_mel)
    out = voc.generate(x, lengths)
    if m64 is not None:
        y, offs = out.grad_fn.sv['y'], voc.packed_plan(out.grad_fn.sv['lens'])[3]
        Fb = voc.n_fft // 2 + 1
        flipped = sum(((torch.exp(y[o:o + m.shape[1], :Fb].t()) > vr.CLAMP) != (m > math.log(vr.CLAMP))).sum().item()
                      for o, m in zip(offs, m64))
    out.backward(r.float())
    if m64 is not None:
        g = {n: p.grad.clone() for n, p in voc.named_parameters()}
        g['mel'] = x.grad.clone()
        return flipped, g
    g = {n: p.grad.clone() for n, p in voc.named_parameters()}
    if want_mel:
        g['mel'] = x.grad.clone()
    return out.detach(), g


# ---- the forward is infer's ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lens", [('small', (40, 40)), ('odd', (40, 40)), ('center', (40, 40)), ('small', (3, 1, 140))])
def test_generate_is_bit_identical_to_infer(native_lib, name, lens):
    voc = _module(name)
    mel = vr.make_mel(len(lens), max(lens), 1, voc.n_mel_channels).to(DEV)
    lengths = list(lens) if len(set(lens)) > 1 else None
    for prec in PRECS:
        voc.precision = prec
        want = voc.infer(mel, lengths)
        got = voc.generate(mel.clone().requires_grad_(True), lengths)
        assert got.grad_fn is not None and got.dtype == torch.float32
        assert torch.equal(got.detach(), want), (name, prec)
        got = voc.generate(mel, lengths)                               # parameters alone require grad
        assert got.grad_fn is not None and torch.equal(got.detach(), want), (name, prec)
        with torch.no_grad():
            assert torch.equal(voc.generate(mel, lengths), want)
    with pytest.raises(ValueError, match="training keeps float32"):
        voc.half().generate(mel)


# ---- gradients against float64 autograd -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lens,seed", [(n, tuple(l), s) for n, l, s in gr.GPU_CASES])
def test_gradients_match_float64_autograd(native_lib, name, lens, seed):
    ref, mel, lengths, r, g64, e32 = _case(name, lens, seed)
    voc = _module(name)
    assert set(g64) == {n for n, _, _ in vr.shapes(ref.config)} | {'mel'}
    with torch.no_grad():
        m64 = [ref.head(ref.backbone(mel[b:b + 1, :, :n].double()))[0][0] for b, n in enumerate(lens)]
    rels = {}
    for prec in PRECS:                                                 # every figure is printed before anything is asserted
        voc.precision = prec
        flipped, g = _grads(voc, mel, lengths, r, m64=m64)
        assert flipped == 0, "%s %s: %d bins on the other side of the clamp than in float64" % (name, prec, flipped)
        assert set(g) == set(g64) and voc.head.istft.window.grad is None
        for k in g64:
            assert g[k].shape == g64[k].shape and g[k].dtype == torch.float32 and torch.isfinite(g[k]).all(), (prec, k)
        rels[prec] = {k: _rel(g[k], g64[k]) for k in g64}
        kw = max(rels[prec], key=rels[prec].get)
        print("\n%s %s %s: worst relative L2 %.3g (%s); float32 autograd there %.3g, its worst %.3g"
              % (name, list(lens), prec, rels[prec][kw], kw, e32[kw], max(e32.values())))
    ratio = {k: rels['fp32'][k] / e32[k] for k in e32}
    kmax = max(ratio, key=ratio.get)
    print("fp32: largest ratio to the float32 autograd %.2f (%s: %.3g against %.3g)"
          % (ratio[kmax], kmax, rels['fp32'][kmax], e32[kmax]))
    for k in e32:
        assert rels['fp32'][k] < 10 * e32[k], (name, 'fp32', k, rels['fp32'][k], e32[k])
    for prec in ('bf16x3', 'bf16'):
        m = MEASURED[(name, lens)][prec]
        for k in e32:
            assert rels[prec][k] < 3 * m, (name, prec, k, rels[prec][k], m)
    if lengths is not None:                                            # zero beyond each utterance's frames
        _, g = _grads(voc, mel, lengths, r)
        for b, n in enumerate(lengths):
            assert not g['mel'][b, :, n:].any() and g['mel'][b, :, :n].any()


def test_ragged_batch_equals_every_utterance_alone(native_lib):
    name, lens, seed = gr.GPU_CASES[-1]
    ref, mel, lengths, r, g64, e32 = _case(name, tuple(lens), seed)
    voc = _module(name)
    _, g = _grads(voc, mel, lengths, r)
    hop = ref.config['hop_length']
    total = None
    for b, n in enumerate(lengths):
        _, ga = _grads(voc, mel[b:b + 1, :, :n].contiguous(), None, r[b:b + 1, :, :hop * n].contiguous())
        assert _rel(g['mel'][b, :, :n], ga['mel'][0]) < 10 * e32['mel'], b
        assert not g['mel'][b, :, n:].any()
        ga.pop('mel')
        total = ga if total is None else {k: total[k] + ga[k] for k in ga}
    for k in total:                                                    # other reduction orders: not bitwise
        assert _rel(g[k], total[k]) < 10 * e32[k], (k, _rel(g[k], total[k]), e32[k])


def test_two_calls_give_the_same_bits(native_lib):
    for name, lens, seed in (gr.GPU_CASES[0], gr.GPU_CASES[-1]):
        ref, mel, lengths, r, _, _ = _case(name, tuple(lens), seed)
        voc = _module(name)
        for prec in PRECS:
            voc.precision = prec
            _, a = _grads(voc, mel, lengths, r)
            _, b = _grads(voc, mel, lengths, r)
            for k in a:
                assert torch.equal(a[k], b[k]), (name, prec, k)


# ---- each kernel alone against torch f32 ------------------------------------------------------------------------------------
def _plan(lens, name='small'):
    from tacotron2_amd.vocos import Vocos
    m = Vocos(**vr.CONFIGS[name])
    rowb0, rowr0, utt, offs, P = m.packed_plan(lens)
    return m, rowb0.to(DEV), rowr0.to(DEV), utt.to(DEV), offs, P


def _image(lens, offs, P, C, seed, scale=1.0):
    """A row image [P][C] with random real rows and zero halos."""
    g = torch.Generator().manual_seed(seed)
    X = torch.zeros(P, C)
    for o, n in zip(offs, lens):
        X[o:o + n] = scale * torch.randn(n, C, generator=g)
    return X.to(DEV)


def _slots(nv, partial, P, n):
    out = torch.empty(n, device=DEV)
    nv.wg_partial_sum(partial, nv.vc_bwd_slots(P), n, out)
    return out


def test_row_kernels_alone_match_torch(native_lib):
    from tacotron2_amd import native as nv
    m, rowb0, rowr0, utt, offs, P = _plan(LENS)
    real = rowb0 >= 0
    slots = nv.vc_bwd_slots(P)
    for i, (D, I) in enumerate(DI):
        g = torch.Generator().manual_seed(30 + i)
        w = (torch.randn(7, D, generator=g) / 7 ** 0.5).to(DEV)
        cb, lw, gamma = [(s * torch.randn(D, generator=g) + o).to(DEV) for s, o in ((0.1, 0.0), (0.1, 1.0), (0.5, 0.0))]
        X = _image(LENS, offs, P, D, 40 + i, 2.0) + 0.5 * real[:, None]
        G, res, dxg, y2 = [_image(LENS, offs, P, D, 50 + 10 * i + j) for j in range(4)]
        u, dh = _image(LENS, offs, P, I, 44 + i, 2.0), _image(LENS, offs, P, I, 48 + i) + 7.0 * (~real)[:, None]
        dz, dz0, dx = [torch.full((P, D), 7.0, device=DEV) for _ in range(3)]
        p_g, p_ln, p_ln0, p_dw = [torch.full((slots * k * D,), 7.0, device=DEV) for k in (1, 2, 2, 8)]
        dh0, y20 = dh.clone(), y2.clone()
        nv.vc_gelu_bwd(u, rowb0, dh)
        nv.vc_gamma_bwd(dxg, gamma, rowb0, y2, p_g)
        nv.vc_ln_bwd(X, w, cb, lw, vr.LN_EPS, rowb0, G, dz, p_ln)
        nv.vc_ln_bwd(X, None, None, lw, vr.LN_EPS, rowb0, G, dz0, p_ln0)
        nv.vc_dw_bwd(dz, X, w, rowb0, res, dx, p_dw)
        for out in (dh, y2, dz, dz0, dx):
            assert not out[~real].any(), "halo rows must be exactly zero"
        R = sum(LENS)
        assert _rel(dh, gr.gelu_bwd(u, dh0) * real[:, None]) < kernel_rel(1)
        want_dy2, want_dg = gr.gamma_bwd(dxg, y20, gamma)
        assert _rel(y2, want_dy2) < kernel_rel(1) and _rel(_slots(nv, p_g, P, D), want_dg) < kernel_rel(R)
        wdz, wdlw, wdlb = gr.ln_bwd(gr.dwconv(X, w, cb, real), lw, G, real)
        assert _rel(dz, wdz) < kernel_rel(D + 7), D
        assert _rel(_slots(nv, p_ln, P, 2 * D), torch.cat([wdlw, wdlb])) < kernel_rel(R + D)
        wdz0, wdlw0, wdlb0 = gr.ln_bwd(X, lw, G, real)
        assert _rel(dz0, wdz0) < kernel_rel(D), D
        assert _rel(_slots(nv, p_ln0, P, 2 * D), torch.cat([wdlw0, wdlb0])) < kernel_rel(R + D)
        wdx, wdw, wdb = gr.dw_bwd(dz, X, w, res, real)
        assert _rel(dx, wdx) < kernel_rel(8)
        assert _rel(_slots(nv, p_dw, P, 8 * D), torch.cat([wdw.flatten(), wdb])) < kernel_rel(R)


@pytest.mark.parametrize("name", ['small', 'odd', 'center', 'V'])
def test_overlap_add_and_polar_backward_alone_match_torch(native_lib, name):
    from tacotron2_amd import native as nv
    from tacotron2_amd.vocos import _pad_cols
    lens = LENS if name != 'center' else [3, 2, 140]                  # 'center': one frame gives no sample
    if name == 'V':
        lens = [3, 1, 20]                                              # 1024 samples a frame: the model below loops on the host
    m, rowb0, rowr0, utt, offs, P = _plan(lens, name)
    real = rowb0 >= 0
    L, hop, Fb = m.n_fft, m.hop, m.n_fft // 2 + 1
    T = m.samples(max(lens))
    d_audio = gr.loss_weights((len(lens), 1, T), 3).float()
    wsq = torch.hann_window(L, periodic=True, dtype=torch.float64) ** 2
    d_frames = torch.full((P, L), 7.0, device=DEV)
    nv.vc_ola_bwd(d_audio.to(DEV), wsq.float().to(DEV), utt, rowb0, rowr0, hop, m.trim(), d_frames)
    want = gr.ola_bwd(d_audio, wsq.float(), lens, offs, P, hop, m.trim())
    assert not d_frames[~real].any()
    assert _rel(d_frames.cpu(), want) < kernel_rel(4), name           # an envelope of at most 4 terms, one division
    nh, ns = _pad_cols(2 * Fb), -(-2 * Fb // 32) * 32
    g = torch.Generator().manual_seed(5)
    Y = torch.cat([torch.randn(P, Fb, generator=g) * 3 + 3, torch.randn(P, Fb, generator=g) * 8, torch.zeros(P, nh - 2 * Fb)],
                  1).to(DEV)
    dS = _image(lens, offs, P, ns, 6)
    dY = torch.full((P, nh), 7.0, device=DEV)
    nv.vc_polar_bwd(Y, Fb, vr.CLAMP, dS, rowb0, dY)
    assert not dY[~real].any() and not dY[:, 2 * Fb:].any()
    e = torch.exp(Y[:, :Fb])
    assert (e[real] > vr.CLAMP).any() and (e[real] < vr.CLAMP).any()
    near = (e / vr.CLAMP - 1.0).abs() < 1e-5                          # exp's last bit may differ between the two sides
    assert not near[real].any()
    want = gr.polar_bwd(Y, dS, Fb) * real[:, None]
    assert not dY[:, :Fb][(e > vr.CLAMP) & real[:, None]].any()
    # phases of up to 30 radians: sincos of a float32 argument x is good to |x| 2^-24 absolutely, a few ulp beside it
    assert _rel(dY[:, :2 * Fb], want) < 8 * kernel_rel(1), name


# ---- parameter updates, training ------------------------------------------------------------------------------------------
def test_an_optimiser_step_is_seen_by_the_next_call(native_lib):
    from tacotron2_amd.optim import FusedAdam
    name, lens, seed = gr.GPU_CASES[0]
    ref, mel, lengths, r, _, _ = _case(name, tuple(lens), seed)
    for make in (lambda ps: FusedAdam(ps, lr=1e-3), lambda ps: torch.optim.SGD(ps, lr=1e-3)):
        voc = _module(name)
        opt = make(list(voc.parameters()))
        before = voc.generate(mel).detach()
        opt.zero_grad()
        voc.generate(mel).backward(r.float())
        opt.step()
        torch.cuda.synchronize()
        after = voc.generate(mel).detach()
        assert not torch.equal(after, before)
        upd = vr.VocosRef(ref.config, {k: v.detach().double() for k, v in voc.state_dict().items()})
        want = upd(mel.double())
        e32 = _rel(upd.float()(mel), want)
        assert _rel(after, want) < 10 * e32, (_rel(after, want), e32)
        assert torch.equal(after, voc.infer(mel))


def test_five_sgd_steps_lower_an_l2_loss(native_lib):
    name, lens, seed = gr.GPU_CASES[0]
    ref, mel, lengths, r, _, _ = _case(name, tuple(lens), seed)
    voc = _module(name)
    target = _module(name, seed=7).infer(mel)
    opt = torch.optim.SGD(voc.parameters(), lr=2e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = F.mse_loss(voc.generate(mel), target)
        losses.append(loss.item())
        loss.backward()
        opt.step()
    print("\nL2 loss over five SGD steps:", " ".join("%.5f" % v for v in losses))
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0]


# ---- allocations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_mel", [False, True])
def test_one_state_one_workspace_one_gradient_block(native_lib, want_mel):
    counts = []
    for name in ('small', 'odd'):
        voc = _module(name)
        mel = vr.make_mel(2, 20, 4, voc.n_mel_channels).to(DEV).requires_grad_(want_mel)
        r = gr.loss_weights((2, 1, voc.samples(20)), 5).float().to(DEV)
        voc.generate(mel, lengths=[20, 11]).backward(r)                # weights packed, plan built, every .grad exists
        torch.cuda.synchronize()
        c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
        out = voc.generate(mel, lengths=[20, 11])
        torch.cuda.synchronize()
        c1 = torch.cuda.memory_stats()["allocation.all.allocated"]
        out.backward(r)
        torch.cuda.synchronize()
        c2 = torch.cuda.memory_stats()["allocation.all.allocated"]
        counts.append((c1 - c0, c2 - c1))
        P = voc.packed_plan([20, 11])[4]
        assert voc.saved_state_bytes(P) == 4 * P * sum(voc.saved_row_widths())
    # the kept state, the workspace and the output; then the gradient block and the backward's workspace
    assert counts == [(3, 2), (3, 2)], counts
