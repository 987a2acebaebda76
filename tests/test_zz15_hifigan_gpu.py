"""The HiFi-GAN generator on the MI355X (csrc/hifigan.hip, csrc/hifigan_post.hip) against the float64 restatement
tests/hifigan_ref.py on the same GPU, each new kernel alone against torch f32, and its batch, size, determinism,
allocation, dtype, checkpoint and CLI contracts; and WaveGlow's bits against the digests of the parent commit.

Relative L2 of the waveform against the float64 restatement, measured on the MI355X (profiles/hifigan_pytest_gpu.txt has the
run; B = 2 at 40 frames on the small geometries, B = 1 at 200 frames on V1):

                 float32 restatement   fp32       bf16x3     bf16
    small1       2.97e-07              4.30e-07   6.63e-06   2.99e-03
    small2       4.42e-07              6.62e-07   1.05e-05   7.50e-03
    small32      3.16e-07              4.27e-07   6.35e-06   2.73e-03
    V1           9.23e-07              1.57e-06   1.56e-05   8.21e-03

MEASURED below holds the bf16x3 and bf16 figures; the bf16x3 and bf16 limits are 3 x the measured value of the geometry, and never above
the sanity bounds 1e-4 / 3e-2.  fp32 is held to 10 x the error the float32 run of the restatement itself shows against
float64 in the same test (the project's rule for WaveGlow's gradients), which does not depend on the code under test."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import hifigan_ref as hr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PRECS = ('fp32', 'bf16x3', 'bf16')
SANITY = {'bf16x3': 1e-4, 'bf16': 3e-2}
# relative L2 against float64, measured (see the module text)
MEASURED = {
    'small1': {'bf16x3': 6.63e-6, 'bf16': 2.99e-3},
    'small2': {'bf16x3': 1.05e-5, 'bf16': 7.50e-3},
    'small32': {'bf16x3': 6.35e-6, 'bf16': 2.73e-3},
    'V1': {'bf16x3': 1.56e-5, 'bf16': 8.21e-3},
}
CASES = [('small1', 2, 40), ('small2', 2, 40), ('small32', 2, 40), ('V1', 1, 200)]
KERNEL_REL = 2e-5       # one product alone against torch f32: two f32 sums of up to 2816 terms in different orders


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


@functools.lru_cache(maxsize=None)
def _ref(name, seed=0):
    return hr.make_ref(name, seed)


def _models(name, seed=0):
    from tacotron2_amd.hifigan import load_hifigan
    ref = _ref(name, seed)
    return ref.to(DEV), load_hifigan({'generator': ref.state_dict(weight_norm=True)}).to(DEV).eval()


@pytest.mark.parametrize("name,B,N", CASES)
def test_matches_float64_restatement_per_precision(native_lib, name, B, N):
    ref, gen = _models(name)
    mel = hr.make_mel(B, N, 1).to(DEV)
    want = ref(mel.double())
    rms = want.pow(2).mean().sqrt().item()
    e32 = _rel(ref.float()(mel), want)
    print("\n%s: output RMS %.3f, float32 restatement %.3g" % (name, rms, e32))
    assert rms > 0.05, "the reference output must not be near zero"
    rels = {}
    for prec in PRECS:
        gen.precision = prec
        got = gen(mel)
        assert got.shape == (B, 1, gen.hop * N) and got.dtype == torch.float32
        rels[prec] = _rel(got, want)
        print("%s %s: relative L2 %.3g" % (name, prec, rels[prec]))
    assert rels['fp32'] < 10 * e32, (name, rels, e32)
    for prec in ('bf16x3', 'bf16'):
        assert rels[prec] < SANITY[prec], (name, prec, rels)
        assert MEASURED[name][prec] is not None, "no measured figure for %s %s" % (name, prec)
        assert rels[prec] < 3 * MEASURED[name][prec], (name, prec, rels)


# ---- each kernel alone -----------------------------------------------------------------------------------------------
def _plan(lens, H):
    from tacotron2_amd.hifigan import Generator
    rowb, rowr, offs = [np.full(H, -1, np.int32)], [np.zeros(H, np.int32)], []
    pos = H
    for b, n in enumerate(lens):
        offs.append(pos)
        rowb += [np.full(n, b, np.int32), np.full(H, -1, np.int32)]
        rowr += [np.arange(n, dtype=np.int32), np.zeros(H, np.int32)]
        pos += n + H
    return torch.from_numpy(np.concatenate(rowb)).to(DEV), torch.from_numpy(np.concatenate(rowr)).to(DEV), offs, pos


def _image(lens, offs, P0, S, C, seed):
    """A row image [P0 S][C] with random real rows, zero halos, and its per-utterance (C, n S) views for torch."""
    g = torch.Generator().manual_seed(seed)
    X = torch.zeros(P0 * S, C)
    utts = []
    for o, n in zip(offs, lens):
        x = torch.randn(C, n * S, generator=g)
        X[o * S:(o + n) * S] = x.t()
        utts.append(x.to(DEV))
    return X.to(DEV), utts


# every (kernel, dilation, channels) of V1 / V2 (type '1': convs1 dilated, convs2 dilation 1) and V3 (type '2')
CONV_CASES = sorted({(k, d, C) for k in (3, 7, 11) for d in (1, 3, 5) for C in (256, 128, 64, 32)} |
                    {(k, d, C) for k, dd in ((3, (1, 2)), (5, (2, 6)), (7, (3, 12))) for d in dd for C in (128, 64, 32)})


def test_conv_kernel_alone_matches_torch_at_every_published_shape(native_lib):
    from tacotron2_amd import native as nv
    from tacotron2_amd.hifigan import pack_conv
    lens, S, H = [3, 1, 2], 32, 2                       # halo 64 rows >= 6 * 7 / ... the widest half-window 36
    rowb0, rowr0, offs, P0 = _plan(lens, H)
    worst = 0.0
    for i, (k, d, C) in enumerate(CONV_CASES):
        g = torch.Generator().manual_seed(100 + i)
        w = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
        b = torch.randn(C, generator=g).to(DEV)
        X, utts = _image(lens, offs, P0, S, C, 200 + i)
        R, _ = _image(lens, offs, P0, S, C, 300 + i)
        wp, bp = pack_conv(w, b, C, C)
        out = torch.full((P0 * S, C), 7.0, device=DEV)
        acc = torch.full((P0 * S, C), 7.0, device=DEV)
        nv.hg_conv(X, wp, bp, k, d, 0.1, None, out, 1.0, False, rowb0, S, 0)                 # plain store
        nv.hg_conv(X, wp, bp, k, d, 0.1, R, acc, 1.0, False, rowb0, S, 0)                    # residual
        nv.hg_conv(X, wp, bp, k, d, 0.1, R, acc, 0.5, True, rowb0, S, 0)                     # fusion sum: += (. + res) / 2
        real = torch.repeat_interleave(rowb0, S) >= 0
        assert not out[~real].any() and not acc[~real].any(), "halo rows must be written as zero"
        for (o, n), x in zip(zip(offs, lens), utts):
            want = F.conv1d(F.leaky_relu(x[None], 0.1), w, b, dilation=d, padding=d * (k - 1) // 2)[0].t()
            got = out[o * S:(o + n) * S]
            r = R[o * S:(o + n) * S]
            rel = max(_rel(got, want), _rel(acc[o * S:(o + n) * S], 1.5 * (want + r)))
            ends = max(_rel(got[:d * k], want[:d * k]), _rel(got[-d * k:], want[-d * k:]))    # both ends of the utterance
            worst = max(worst, rel, ends)
            assert rel < KERNEL_REL and ends < KERNEL_REL, (k, d, C, rel, ends)
    print("\nconv alone, %d shapes: worst relative L2 %.3g" % (len(CONV_CASES), worst))


UP_CASES = [(512, 256, 16, 8), (256, 128, 16, 8), (128, 64, 4, 2), (64, 32, 4, 2),          # V1
            (128, 64, 16, 8), (64, 32, 16, 8), (32, 16, 4, 2), (16, 8, 4, 2),               # V2 (16 and 8 run padded to 32)
            (256, 128, 16, 8), (128, 64, 16, 8), (64, 32, 8, 4)]                            # V3


def test_upsample_kernel_alone_matches_torch_at_every_published_stage(native_lib):
    from tacotron2_amd import native as nv
    from tacotron2_amd.hifigan import _ce, pack_up
    lens, S, H = [5, 1, 3], 2, 1
    rowb0, rowr0, offs, P0 = _plan(lens, H)
    worst = 0.0
    for i, (ci, co, ku, u) in enumerate(UP_CASES):
        g = torch.Generator().manual_seed(400 + i)
        w = (torch.randn(ci, co, ku, generator=g) / (ci * ku / u) ** 0.5).to(DEV)
        b = torch.randn(co, generator=g).to(DEV)
        cie, coe = _ce(ci), _ce(co)
        X, utts = _image(lens, offs, P0, S, cie, 500 + i)
        X[:, ci:] = 0
        wp, bp = pack_up(w, b, u, cie, coe)
        out = torch.full((P0 * S * u, coe), 7.0, device=DEV)
        nv.hg_upsample(X, wp, bp, ku, u, 0.1, out, rowb0, S, 0)
        real = torch.repeat_interleave(rowb0, S * u) >= 0
        assert not out[~real].any() and not out[:, co:].any()
        for (o, n), x in zip(zip(offs, lens), utts):
            want = F.conv_transpose1d(F.leaky_relu(x[None, :ci], 0.1), w, b, stride=u, padding=(ku - u) // 2)[0].t()
            got = out[o * S * u:(o + n) * S * u, :co]
            rel = _rel(got, want)
            first, last = _rel(got[0::u], want[0::u]), _rel(got[u - 1::u], want[u - 1::u])  # first and last phase
            ends = max(_rel(got[:u], want[:u]), _rel(got[-u:], want[-u:]))
            worst = max(worst, rel, first, last, ends)
            assert max(rel, first, last, ends) < KERNEL_REL, (ci, co, ku, u, rel, first, last, ends)
    print("\nupsample alone, %d stages: worst relative L2 %.3g" % (len(UP_CASES), worst))


def test_conv_post_and_mel_packing_alone_match_torch(native_lib):
    from tacotron2_amd import native as nv
    lens, S, H = [3, 1, 2], 256, 1
    rowb0, rowr0, offs, P0 = _plan(lens, H)
    for C in (32, 64):
        g = torch.Generator().manual_seed(600 + C)
        w = (0.2 * torch.randn(1, C, 7, generator=g)).to(DEV)
        b = torch.randn(1, generator=g).to(DEV)
        X, utts = _image(lens, offs, P0, S, C, 700 + C)
        out = torch.zeros(3, 1, 3 * S, device=DEV)
        nv.hg_post(X, w[0].t().contiguous(), b, 0.01, rowb0, rowr0, S, out)
        for bi, ((o, n), x) in enumerate(zip(zip(offs, lens), utts)):
            # two float32 sums of 7 C terms in different orders: held to 10 x the error torch's float32 shows against float64
            want = torch.tanh(F.conv1d(F.leaky_relu(x[None].double()), w.double(), b.double(), padding=3))[0, 0]
            e32 = (torch.tanh(F.conv1d(F.leaky_relu(x[None]), w, b, padding=3))[0, 0] - want).abs().max().item()
            err = (out[bi, 0, :n * S] - want).abs().max().item()
            print("conv_post C=%d: max abs error %.3g, torch float32 %.3g" % (C, err, e32))
            assert e32 > 0 and err < 10 * e32, (C, err, e32)
            assert not out[bi, 0, n * S:].any()
    mel = hr.make_mel(3, 3, 8).to(DEV)
    img = torch.full((P0, 96), 7.0, device=DEV)
    nv.hg_pack_mel(mel, rowb0, rowr0, img)
    assert not img[rowb0 < 0].any() and not img[:, 80:].any()
    for bi, (o, n) in enumerate(zip(offs, lens)):
        assert torch.equal(img[o:o + n, :80], mel[bi, :, :n].t())


# ---- batch, size, determinism, allocations ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_ragged_equals_alone_bitwise(native_lib, prec):
    from tacotron2_amd.synth import synth_lengths
    _, gen = _models('V1')
    gen.precision = prec
    lens = [int(n) for n in synth_lengths(16, 1234)[1]]
    N = max(lens)
    mel = hr.make_mel(16, N, 2).to(DEV)
    out = gen.infer(mel, lengths=lens)
    assert out.shape == (16, 1, 256 * N)
    for b, n in enumerate(lens):
        alone = gen.infer(mel[b:b + 1, :, :n])
        assert torch.equal(out[b, 0, :256 * n], alone[0, 0]), (prec, b)
        assert not out[b, 0, 256 * n:].any(), (prec, b)
    assert torch.equal(out, gen.infer(mel, lengths=lens)), "two calls must give the same bits"


def test_more_than_65535_frame_rows_and_2_pow_24_sample_rows(native_lib):
    """66,000 frames: stage 0 has more than 65,535 rows and the last stage 16.9 M (> 2^24).  The head and the tail of the long
    utterance equal the same frames vocoded as short utterances, bit for bit, away from the cut (the receptive field of
    V1 is under 64 frames): rows far beyond 2^24 are addressed and masked like the first ones."""
    _, gen = _models('V1')
    N, n, margin = 66000, 1000, 64
    mel = hr.make_mel(1, N, 3).to(DEV)
    out = gen.infer(mel)
    assert out.shape == (1, 1, 256 * N) and 256 * N > 2 ** 24 and bool(torch.isfinite(out).all())
    head = gen.infer(mel[:, :, :n])
    tail = gen.infer(mel[:, :, -n:])
    keep = 256 * (n - margin)
    assert torch.equal(out[0, 0, :keep], head[0, 0, :keep])
    assert torch.equal(out[0, 0, -keep:], tail[0, 0, -keep:])
    assert out[0, 0, -keep:].abs().max().item() > 0.05


def test_allocation_count_does_not_grow_with_stages_or_blocks(native_lib):
    counts = []
    for name in ('small32', 'small1', 'small2', 'V1'):          # 20 / 26 / 14 / 76 launches in the stage loop
        _, gen = _models(name)
        mel = hr.make_mel(2, 20, 4).to(DEV)
        gen.infer(mel, lengths=[20, 11])                        # weights packed, plan built
        torch.cuda.synchronize()
        c0 = torch.cuda.memory_stats()["allocation.all.allocated"]
        gen.infer(mel, lengths=[20, 11])
        torch.cuda.synchronize()
        counts.append(torch.cuda.memory_stats()["allocation.all.allocated"] - c0)
    assert len(set(counts)) == 1 and counts[0] <= 3, counts    # the workspace, the output (and the mel's f32 copy, if any)


# ---- other surface ------------------------------------------------------------------------------------------------------
def test_half_mode_and_low_precision_mels(native_lib):
    ref, gen = _models('small1', seed=5)
    mel = hr.make_mel(2, 20, 6).to(DEV)
    gen.precision = 'bf16'
    base = gen(mel.half().float())
    gen = gen.half()
    assert gen.precision == 'bf16' and gen.conv_pre.weight.dtype == torch.float32
    out = gen(mel.half())
    assert out.dtype == torch.float16 and torch.equal(out, base.half())
    rel = _rel(out.float(), ref(mel.half().double()))
    print("\n.half(): relative L2 %.3g" % rel)
    assert rel < SANITY['bf16']
    gen = gen.float()
    assert gen.precision == 'fp32'
    want16 = gen(mel.bfloat16().float())
    assert torch.equal(gen(mel.bfloat16()), want16) and want16.dtype == torch.float32


def test_checkpoint_round_trip_both_forms_and_notebook_call(native_lib, tmp_path):
    from tacotron2_amd.hifigan import load_hifigan
    ref = _ref('small2', 7)
    mel = hr.make_mel(1, 16, 8).to(DEV)
    outs = []
    for form, sd in (("normed", ref.state_dict(weight_norm=True)), ("folded", ref.state_dict())):
        p = str(tmp_path / (form + ".pt"))
        torch.save({'generator': {k: v.float() for k, v in sd.items()}}, p)
        audio = load_hifigan(p).cuda().eval()(mel)
        assert audio.shape == (1, 1, 16 * 8)                    # small2: 4 x 2 samples per frame
        outs.append(audio)
    assert _rel(outs[0], outs[1]) < 1e-6                        # the fold in float32 against the float32 of the float64 fold
    assert _rel(outs[1], ref.to(DEV)(mel.double())) < 1e-5


def test_cli_hifigan_writes_wavs(native_lib, tmp_path):
    from scipy.io import wavfile
    ref = _ref('V2', 9)
    ckpt = str(tmp_path / "g.pt")
    torch.save({'generator': {k: v.float() for k, v in ref.state_dict(weight_norm=True).items()}}, ckpt)
    lens, files = [12, 7], []
    for i, n in enumerate(lens):
        p = str(tmp_path / ("m%d.npy" % i))
        np.save(p, hr.make_mel(1, n, 10 + i)[0].numpy())
        files.append(p)
    out = str(tmp_path / "wav")
    env = dict(os.environ, PYTHONPATH=gu.ROOT)
    subprocess.check_call([sys.executable, "-m", "tacotron2_amd.vocode"] + files + ["-o", out, "--hifigan", ckpt,
                                                                                      "--precision", "bf16x3"], env=env, cwd=gu.ROOT)
    for i, n in enumerate(lens):
        sr, x = wavfile.read(os.path.join(out, "m%d.wav" % i))
        assert sr == 22050 and x.dtype == np.int16 and x.shape == (256 * n,) and np.abs(x).max() > 1000


# ---- WaveGlow is untouched -----------------------------------------------------------------------------------------------------
def test_waveglow_bits_equal_the_parent_commits(native_lib):
    sys.path.insert(0, gu.GOLDEN_DIR)
    try:
        import make_golden_waveglow_digests as mk
    finally:
        sys.path.remove(gu.GOLDEN_DIR)
    with open(os.path.join(gu.GOLDEN_DIR, "waveglow_digests.json")) as fh:
        want = json.load(fh)
    got = mk.digests()
    assert set(got) == set(want) and len(want) == 12
    assert got == want, sorted(k for k in want if got[k] != want[k])


# ---- the shared tile loop (csrc/rowmma.h) moves no bit of the generator --------------------------------------------------------
def test_hifigan_bits_equal_the_digests_from_before_the_shared_tile_loop(native_lib):
    """tests/golden/vocoder_digests.json was written by the commit before the three vocoders' tile loops became one: the small
    generators full and ragged, V1 ragged, and hg_conv / hg_upsample alone at C = 32, 64 and 128, per precision."""
    sys.path.insert(0, gu.GOLDEN_DIR)
    try:
        import make_golden_vocoder_digests as mk
    finally:
        sys.path.remove(gu.GOLDEN_DIR)
    with open(os.path.join(gu.GOLDEN_DIR, "vocoder_digests.json")) as fh:
        want = json.load(fh)["hifigan"]
    got = mk.digests_hifigan()
    assert set(got) == set(want) and len(want) == 51
    assert got == want, sorted(k for k in want if got[k] != want[k])
