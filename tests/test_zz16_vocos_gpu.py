"""The Vocos vocoder on the MI355X (csrc/vocos.hip, csrc/vocos_rows.hip) against the float64 restatement tests/vocos_ref.py on
the same GPU, each new kernel alone against torch f32, and its batch, size, determinism, allocation, dtype, weight-update and
CLI contracts.

Relative L2 of the waveform against the float64 restatement, measured on the MI355X (profiles/vocos_pytest_gpu.txt has the
run; B = 2 at 40 frames on the small geometries, B = 1 at 64 frames on V):

                 float32 restatement   fp32       bf16x3     bf16
    small        4.11e-07              5.87e-07   1.58e-05   6.19e-03
    odd          1.34e-06              1.99e-06   2.40e-05   1.02e-02
    center       4.12e-07              5.85e-07   1.55e-05   6.11e-03
    V            1.85e-06              2.45e-06   2.20e-05   7.88e-03

MEASURED below holds the bf16x3 and bf16 figures; their limits are 3 x the measured value of the geometry, and never above the
sanity bounds 1e-4 / 3e-2.  fp32 is held to 10 x the error the float32 run of the restatement itself shows against float64 in
the same test, which does not depend on the code under test.  With 'bf16' only the two products of every block run in bf16:
the head product and the inverse DFT stay split-bf16, since a phase error goes straight into the waveform."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import vocos_ref as vr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PRECS = ('fp32', 'bf16x3', 'bf16')
SANITY = {'bf16x3': 1e-4, 'bf16': 3e-2}
# relative L2 against float64, measured (see the module text)
MEASURED = {
    'small': {'bf16x3': 1.58e-5, 'bf16': 6.19e-3},
    'odd': {'bf16x3': 2.40e-5, 'bf16': 1.02e-2},
    'center': {'bf16x3': 1.55e-5, 'bf16': 6.11e-3},
    'V': {'bf16x3': 2.20e-5, 'bf16': 7.88e-3},
}
CASES = [('small', 2, 40), ('odd', 2, 40), ('center', 2, 40), ('V', 1, 64)]
DI = [(64, 192), (96, 160), (512, 1536)]            # (D, I) of the geometries above
U = 2.0 ** -24


def kernel_rel(K):
    """One kernel alone against torch f32, relative L2: both sides round a sum of K terms of random sign, in different orders.
    The partial sums grow like sqrt(k), so the rounding errors (u sqrt(k) each, u = 2^-24) add up to about u K / sqrt 2
    against a result of size sqrt K: u sqrt(K / 2) a side, u sqrt K for the two.  Four times that, plus 4 u a side for the
    element-wise epilogue (bias, erf / exp / sincos, the scale), covers sums whose terms are not of random sign."""
    return 4.0 * (K ** 0.5 + 4.0) * U


def product_rel(K, prec):
    """The products alone at the lower precisions, relative L2 against torch f32.  The error of every term is independent of
    the others, so a sum of K terms of random sign keeps the relative error of one term, whatever K.  bf16: each operand is
    rounded to 8 bits, relative error uniform in +-2^-9, rms 2^-9 / sqrt 3; two operands: sqrt(2 / 3) 2^-9 = 1.6e-3.
    Split-bf16 x 3: the low half is the bf16 rounding of a residual below 2^-9, so an operand is off by 2^-18 / sqrt 3 rms,
    two by sqrt(2 / 3) 2^-18, and the dropped low x low term adds 2^-18 / 3: 4.4e-6 together.  Four times the figure, as in
    kernel_rel, plus kernel_rel(K) for the f32 accumulation and the epilogue that both modes share with the exact one."""
    per_term = {1: (2.0 / 3.0) ** 0.5 * 2.0 ** -18 + 2.0 ** -18 / 3.0, 2: (2.0 / 3.0) ** 0.5 * 2.0 ** -9}[prec]
    return 4.0 * per_term + kernel_rel(K)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


@functools.lru_cache(maxsize=None)
def _ref(name, seed=0):
    return vr.make_ref(name, seed)


def _models(name, seed=0):
    from tacotron2_amd.vocos import load_vocos
    ref = _ref(name, seed)
    c = ref.config
    return ref.to(DEV), load_vocos(ref.state_dict(), hop_length=c['hop_length'], padding=c['padding']).to(DEV).eval()


def _mel(ref, B, N, seed):
    return vr.make_mel(B, N, seed, ref.config['n_mel_channels']).to(DEV)


@pytest.mark.parametrize("name,B,N", CASES)
def test_matches_float64_restatement_per_precision(native_lib, name, B, N):
    ref, voc = _models(name)
    mel = _mel(ref, B, N, 1)
    want = ref(mel.double())
    rms = want.pow(2).mean().sqrt().item()
    e32 = _rel(ref.float()(mel), want)
    print("\n%s: output RMS %.3f, float32 restatement %.3g" % (name, rms, e32))
    assert rms > 0.05, "the reference output must not be near zero"
    rels = {}
    for prec in PRECS:
        voc.precision = prec
        got = voc(mel)
        assert got.shape == (B, 1, voc.samples(N)) == want.shape and got.dtype == torch.float32
        rels[prec] = _rel(got, want)
        print("%s %s: relative L2 %.3g" % (name, prec, rels[prec]))
    assert rels['fp32'] < 10 * e32, (name, rels, e32)
    for prec in ('bf16x3', 'bf16'):
        assert rels[prec] < SANITY[prec], (name, prec, rels)
        assert MEASURED[name][prec] is not None, "no measured figure for %s %s" % (name, prec)
        assert rels[prec] < 3 * MEASURED[name][prec], (name, prec, rels)


# ---- each kernel alone -----------------------------------------------------------------------------------------------
LENS = [3, 1, 140]                                   # more than one 128-row tile, a one-frame utterance


def _plan(lens):
    from tacotron2_amd.vocos import Vocos
    rowb0, rowr0, utt, offs, P = Vocos(**vr.CONFIGS['small']).packed_plan(lens)
    return rowb0.to(DEV), rowr0.to(DEV), utt.to(DEV), offs, P


def _image(lens, offs, P, C, seed, scale=1.0):
    """A row image [P][C] with random real rows and zero halos."""
    g = torch.Generator().manual_seed(seed)
    X = torch.zeros(P, C)
    for o, n in zip(offs, lens):
        X[o:o + n] = scale * torch.randn(n, C, generator=g)
    return X.to(DEV)


def test_dwconv_layernorm_kernel_alone_matches_torch(native_lib):
    from tacotron2_amd import native as nv
    rowb0, rowr0, utt, offs, P = _plan(LENS)
    for i, (D, _) in enumerate(DI):
        g = torch.Generator().manual_seed(10 + i)
        w = (torch.randn(D, 1, 7, generator=g) / 7 ** 0.5).to(DEV)
        cb, lw, lb = [(s * torch.randn(D, generator=g) + o).to(DEV) for s, o in ((0.1, 0.0), (0.1, 1.0), (0.1, 0.0))]
        X = _image(LENS, offs, P, D, 20 + i, 2.0) + 0.5 * (rowb0 >= 0)[:, None]
        out, ln = torch.full((P, D), 7.0, device=DEV), torch.full((P, D), 7.0, device=DEV)
        nv.vc_dwln(X, w[:, 0, :].t().contiguous(), cb, lw, lb, 1e-6, rowb0, out)
        nv.vc_dwln(X, None, None, lw, lb, 1e-6, rowb0, ln)                                   # zero taps: LayerNorm alone
        assert not out[rowb0 < 0].any() and not ln[rowb0 < 0].any(), "halo rows must be written as zero"
        for o, n in zip(offs, LENS):
            x = X[o:o + n].t()[None]
            want = F.layer_norm(F.conv1d(x, w, cb, padding=3, groups=D)[0].t(), (D,), lw, lb, 1e-6)
            want_ln = F.layer_norm(X[o:o + n], (D,), lw, lb, 1e-6)
            rel, rel_ln = _rel(out[o:o + n], want), _rel(ln[o:o + n], want_ln)
            print("dwconv + LayerNorm D=%d n=%d: relative L2 %.3g, LayerNorm alone %.3g" % (D, n, rel, rel_ln))
            assert rel < kernel_rel(D + 7) and rel_ln < kernel_rel(D), (D, n, rel, rel_ln)


@pytest.mark.parametrize("prec", [0, 1, 2])
def test_product_kernels_alone_match_torch(native_lib, prec):
    from tacotron2_amd import native as nv
    rowb0, rowr0, utt, offs, P = _plan(LENS)
    real = rowb0 >= 0
    for i, (D, I) in enumerate(DI):
        g = torch.Generator().manual_seed(30 + i)
        w1, b1 = (torch.randn(I, D, generator=g) / D ** 0.5).to(DEV), (0.1 * torch.randn(I, generator=g)).to(DEV)
        w2, b2 = (torch.randn(D, I, generator=g) / I ** 0.5).to(DEV), (0.1 * torch.randn(D, generator=g)).to(DEV)
        gamma = (0.5 * torch.randn(D, generator=g)).to(DEV)
        X = _image(LENS, offs, P, D, 40 + i, 3.0)                       # pwconv1 outputs span about +-8: both GELU tails
        R = _image(LENS, offs, P, D, 50 + i)
        h = torch.full((P, I), 7.0, device=DEV)
        nv.vc_linear(X, w1, b1, 'gelu', None, None, h, rowb0, prec)
        pre = F.linear(X, w1, b1)
        assert pre[real].min().item() < -8 and pre[real].max().item() > 8
        want_h = F.gelu(pre)
        y = R.clone()
        nv.vc_linear(h, w2, b2, 'residual', gamma, y, y, rowb0, prec)                        # in place, as the layer loop
        want_y = R + gamma * F.linear(h, w2, b2)
        plain = torch.full((P, D), 7.0, device=DEV)
        nv.vc_linear(h, w2, None, None, None, None, plain, rowb0, prec)
        assert not h[~real].any() and not y[~real].any() and not plain[~real].any(), "halo rows must be written as zero"
        rels = (_rel(h[real], want_h[real]), _rel(y[real], want_y[real]), _rel(plain[real], F.linear(h, w2)[real]))
        print("products D=%d I=%d precision %d: GELU %.3g, gamma / residual %.3g, plain %.3g" % ((D, I, prec) + rels))
        tol = kernel_rel if prec == 0 else (lambda K: product_rel(K, prec))
        assert rels[0] < tol(D) and rels[1] < tol(I) and rels[2] < tol(I), (D, I, prec, rels, tol(D), tol(I))


def test_polar_kernel_alone_matches_torch(native_lib):
    from tacotron2_amd import native as nv
    rowb0, rowr0, utt, offs, P = _plan(LENS)
    real = rowb0 >= 0
    for F_ in (33, 65, 513):
        ld, lds = -(-2 * F_ // 128) * 128, -(-2 * F_ // 32) * 32
        Y = torch.full((P, ld), 3.0, device=DEV)
        Y[:, :F_] = torch.linspace(-8.0, 8.0, P * F_, device=DEV).view(P, F_)
        Y[:, F_:2 * F_] = torch.linspace(-20.0, 20.0, P * F_, device=DEV).view(F_, P).t()
        S = torch.full((P, lds), 7.0, device=DEV)
        nv.vc_polar(Y, F_, 100.0, rowb0, S)
        mag = torch.clamp(torch.exp(Y[:, :F_]), max=100.0)
        want = torch.stack([mag * torch.cos(Y[:, F_:2 * F_]), mag * torch.sin(Y[:, F_:2 * F_])], 2).view(P, 2 * F_)
        assert not S[~real].any() and not S[:, 2 * F_:].any()
        assert (mag[real] == 100.0).any() and (mag[real] < 0.01).any()
        rel = _rel(S[real][:, :2 * F_], want[real])
        worst = ((S[real][:, :2 * F_] - want[real]).abs() / mag[real].repeat_interleave(2, 1)).max().item()
        print("polar F=%d: relative L2 %.3g, worst error over the magnitude %.3g" % (F_, rel, worst))
        assert rel < kernel_rel(1) and worst < 16 * U, (F_, rel, worst)     # exp, sincos and a product: a few ulp each side


@pytest.mark.parametrize("padding", ['same', 'center'])
def test_inverse_dft_and_overlap_add_alone_match_torch(native_lib, padding):
    from tacotron2_amd import native as nv
    from tacotron2_amd.vocos import inverse_basis
    lens = [3, 1, 140] if padding == 'same' else [3, 2, 140]
    rowb0, rowr0, utt, offs, P = _plan(lens)
    for L, hop in ((64, 16), (128, 32), (1024, 256)):
        F_ = L // 2 + 1
        win = torch.hann_window(L, periodic=True)
        basis, wsq = inverse_basis(win).to(DEV), (win.double() ** 2).float().to(DEV)
        S = _image(lens, offs, P, basis.shape[1], L)
        S[:, 2 * F_:] = 0
        frames = torch.full((P, L), 7.0, device=DEV)
        nv.vc_linear(S, basis, None, None, None, None, frames, rowb0, 0)
        trim = (L - hop) // 2 if padding == 'same' else L // 2
        per = hop * max(lens) if padding == 'same' else hop * (max(lens) - 1)
        out = torch.full((len(lens), 1, per), 7.0, device=DEV)
        nv.vc_ola(frames, wsq, utt, hop, trim, out)
        for b, (o, n) in enumerate(zip(offs, lens)):
            rows = S[o:o + n, :2 * F_].view(n, F_, 2)
            spec = torch.complex(rows[:, :, 0], rows[:, :, 1]).t()[None]
            want = vr.istft(spec, win.to(DEV), hop, padding)[0]
            T = want.numel()
            assert T == (hop * n if padding == 'same' else hop * (n - 1))
            rel = _rel(out[b, 0, :T], want)
            print("inverse DFT + overlap-add %s n_fft=%d n=%d: relative L2 %.3g" % (padding, L, n, rel))
            assert rel < kernel_rel(2 * F_), (padding, L, n, rel)
            assert not out[b, 0, T:].any(), "zero beyond the utterance"


# ---- batch, size, determinism, allocations ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ['small', 'odd'])
def test_ragged_equals_alone_bitwise(native_lib, name, prec):
    ref, voc = _models(name)
    voc.precision = prec
    lens = [1, 7, 40]
    mel = _mel(ref, 3, 40, 2)
    out = voc.infer(mel, lengths=lens)
    assert out.shape == (3, 1, voc.hop * 40)
    for b, n in enumerate(lens):
        alone = voc.infer(mel[b:b + 1, :, :n])
        assert torch.equal(out[b, 0, :voc.hop * n], alone[0, 0]), (name, prec, b)
        assert not out[b, 0, voc.hop * n:].any(), (name, prec, b)
        assert alone.abs().max().item() > 0.05
    assert torch.equal(out, voc.infer(mel, lengths=lens)), "two calls must give the same bits"


def test_long_utterance_of_70000_frames(native_lib):
    """70,000 frame rows: 17,500 workgroups of the row kernels and 547 row tiles of the products in grid.x, 1.12 M samples."""
    ref, voc = _models('small')
    N = 70000
    mel = _mel(ref, 1, N, 3)
    want = ref(mel.double())
    e32 = _rel(ref.float()(mel), want)
    got = voc.infer(mel)
    rel = _rel(got, want)
    tail = _rel(got[..., -4096:], want[..., -4096:])
    print("\n70,000 frames: relative L2 %.3g (last 4096 samples %.3g), float32 restatement %.3g" % (rel, tail, e32))
    assert got.shape == (1, 1, 16 * N) and rel < 10 * e32 and tail < 10 * e32


def test_one_allocation_beyond_the_output(native_lib):
    counts = []
    for name in ('small', 'odd', 'V'):                          # 2 / 3 / 8 blocks
        ref, voc = _models(name)
        mel = _mel(ref, 2, 20, 4)
        voc.infer(mel, lengths=[20, 11])                        # weights packed, plan built
        torch.cuda.synchronize()
        c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
        voc.infer(mel, lengths=[20, 11])
        torch.cuda.synchronize()
        counts.append(torch.cuda.memory_stats()["allocation.all.allocated"] - c0)
    assert counts == [2, 2, 2], counts                          # the workspace and the output


def test_half_mode_low_precision_mels_and_weight_update(native_lib):
    from tacotron2_amd.vocos import load_vocos
    ref, voc = _models('small', seed=5)
    mel = _mel(ref, 2, 20, 6)
    voc.precision = 'bf16'
    base = voc(mel.half().float())
    voc = voc.half()
    assert voc.precision == 'bf16' and voc.head.out.weight.dtype == torch.float32
    out = voc(mel.half())
    assert out.dtype == torch.float16 and torch.equal(out, base.half())
    voc = voc.float()
    assert voc.precision == 'fp32'
    want16 = voc(mel.bfloat16().float())
    assert torch.equal(voc(mel.bfloat16()), want16) and want16.dtype == torch.float32
    # a weight update invalidates the pack: the next call equals a model loaded from the updated weights
    before = voc(mel)
    with torch.no_grad():
        voc.backbone.convnext[1].gamma.mul_(2.0)
        voc.head.out.bias.add_(0.25)
    after = voc(mel)
    c = ref.config
    fresh = load_vocos({k: v.cpu() for k, v in voc.state_dict().items()}, hop_length=c['hop_length']).to(DEV)
    assert not torch.equal(after, before) and torch.equal(after, fresh(mel))


def test_cli_vocos_writes_wavs(native_lib, tmp_path):
    from scipy.io import wavfile
    ref = vr.make_ref(dict(vr.CONFIGS['V'], dim=64, intermediate_dim=96, num_layers=1), 9)
    ckpt = str(tmp_path / "v.pt")
    sd = {k: v.float() for k, v in ref.state_dict().items()}
    sd['feature_extractor.mel_spec.spectrogram.window'] = torch.zeros(1024)
    torch.save({'state_dict': sd}, ckpt)
    lens, files = [12, 7], []
    for i, n in enumerate(lens):
        p = str(tmp_path / ("m%d.npy" % i))
        np.save(p, vr.make_mel(1, n, 10 + i)[0].numpy())
        files.append(p)
    out = str(tmp_path / "wav")
    env = dict(os.environ, PYTHONPATH=gu.ROOT)
    subprocess.check_call([sys.executable, "-m", "tacotron2_amd.vocode"] + files + ["-o", out, "--vocos", ckpt,
                                                                                      "--precision", "bf16x3"], env=env, cwd=gu.ROOT)
    for i, n in enumerate(lens):
        sr, x = wavfile.read(os.path.join(out, "m%d.wav" % i))
        assert sr == 22050 and x.dtype == np.int16 and x.shape == (256 * n,) and np.abs(x).max() > 1000


# ---- the shared tile loop (csrc/rowmma.h) moves no bit of the vocoder ----------------------------------------------------------
def test_vocos_bits_equal_the_digests_from_before_the_shared_tile_loop(native_lib):
    """tests/golden/vocoder_digests.json was written by the commit before the three vocoders' tile loops became one: 'small' and
    'odd' full and ragged, and vc_linear's three epilogues alone at every (D, I) of DI (BN = 64, 32 and 128), per precision."""
    sys.path.insert(0, gu.GOLDEN_DIR)
    try:
        import make_golden_vocoder_digests as mk
    finally:
        sys.path.remove(gu.GOLDEN_DIR)
    with open(os.path.join(gu.GOLDEN_DIR, "vocoder_digests.json")) as fh:
        want = json.load(fh)["vocos"]
    got = mk.digests_vocos()
    assert set(got) == set(want) and len(want) == 39
    assert got == want, sorted(k for k in want if got[k] != want[k])
