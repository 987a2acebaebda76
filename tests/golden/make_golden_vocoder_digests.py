"""sha256 of the HiFi-GAN and Vocos outputs on an MI355X, per precision: the whole generators, full and ragged, and the
product kernels alone at one shape per tile instantiation (BN = 128 / 64 / 32), so that a moved bit is localised.

    python tests/golden/make_golden_vocoder_digests.py [--root TREE] [--out tests/golden/vocoder_digests.json]

``--root`` selects the checkout whose ``tacotron2_amd`` is imported (default: this one), so the fixture can be written from
the commit BEFORE a change and compared with the commit after it (tests/test_zz15_hifigan_gpu.py and
tests/test_zz16_vocos_gpu.py do: the three vocoders share one MFMA tile loop, csrc/rowmma.h, and a change to it must not move
a bit of any of them).  ``_meta.source_sha1`` is ``t2amd_source_sha1()`` of the library that wrote the fixture.

The shapes are those of the two files' ``test_ragged_equals_alone_bitwise`` and "alone" tests: a 1-frame utterance, halo rows
inside a tile, C = 128, 64 and 32, and the polyphase upsample, whose first and last phases take different tap bases."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PRECS = ('fp32', 'bf16x3', 'bf16')


def _sha(*tensors):
    import numpy as np
    h = hashlib.sha256()
    for t in tensors:
        a = np.ascontiguousarray(t.detach().float().cpu().numpy())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _hg_plan(lens, H, dev):
    """tests/test_zz15_hifigan_gpu.py's _plan: H halo rows before, between and after the utterances."""
    import numpy as np
    import torch
    rowb, offs, pos = [np.full(H, -1, np.int32)], [], H
    for b, n in enumerate(lens):
        offs.append(pos)
        rowb += [np.full(n, b, np.int32), np.full(H, -1, np.int32)]
        pos += n + H
    return torch.from_numpy(np.concatenate(rowb)).to(dev), offs, pos


def _image(lens, offs, P0, S, C, seed, dev):
    """A row image [P0 S][C] with random real rows and zero halos."""
    import torch
    g = torch.Generator().manual_seed(seed)
    X = torch.zeros(P0 * S, C)
    for o, n in zip(offs, lens):
        X[o * S:(o + n) * S] = torch.randn(n * S, C, generator=g)
    return X.to(dev)


def digests_hifigan():
    """{'<entry>/<precision>': sha256}; needs cuda:0 and ``tacotron2_amd`` / tests/hifigan_ref.py importable."""
    import torch
    import hifigan_ref as hr
    from tacotron2_amd import native as nv
    from tacotron2_amd.hifigan import load_hifigan, pack_conv, pack_up
    from tacotron2_amd.synth import synth_lengths
    dev = torch.device("cuda", 0)
    out = {}
    # the small seeded generators (C = 64 -> 32 -> 16 padded to 32, both resblock types; C = 128 -> 64 -> 32), full and ragged
    for name in ('small1', 'small2', 'small32'):
        ref = hr.make_ref(name, 0)
        gen = load_hifigan({'generator': ref.state_dict(weight_norm=True)}).to(dev).eval()
        mel = hr.make_mel(3, 40, 2).to(dev)
        for prec in PRECS:
            gen.precision = prec
            out['%s/infer/%s' % (name, prec)] = _sha(gen.infer(mel))
            out['%s/infer_ragged/%s' % (name, prec)] = _sha(gen.infer(mel, lengths=[1, 7, 40]))
    # test_ragged_equals_alone_bitwise as it is: V1, 16 utterances
    ref = hr.make_ref('V1', 0)
    gen = load_hifigan({'generator': ref.state_dict(weight_norm=True)}).to(dev).eval()
    lens = [int(n) for n in synth_lengths(16, 1234)[1]]
    mel = hr.make_mel(16, max(lens), 2).to(dev)
    for prec in PRECS:
        gen.precision = prec
        out['V1/infer_ragged/' + prec] = _sha(gen.infer(mel, lengths=lens))
    # hg_conv alone: k = 7, d = 3 at C = 32 / 64 / 128 (BN = 32 / 64 / 128), plain store, residual, and the fusion sum
    lens, S, H = [3, 1, 2], 32, 2
    rowb0, offs, P0 = _hg_plan(lens, H, dev)
    k, d = 7, 3
    for C in (32, 64, 128):
        g = torch.Generator().manual_seed(100 + C)
        w = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(dev)
        b = torch.randn(C, generator=g).to(dev)
        X = _image(lens, offs, P0, S, C, 200 + C, dev)
        R = _image(lens, offs, P0, S, C, 300 + C, dev)
        wp, bp = pack_conv(w, b, C, C)
        for pi, prec in enumerate(PRECS):
            store = torch.full((P0 * S, C), 7.0, device=dev)
            acc = torch.full((P0 * S, C), 7.0, device=dev)
            nv.hg_conv(X, wp, bp, k, d, 0.1, None, store, 1.0, False, rowb0, S, pi)
            nv.hg_conv(X, wp, bp, k, d, 0.1, R, acc, 1.0, False, rowb0, S, pi)
            res = acc.clone()
            nv.hg_conv(X, wp, bp, k, d, 0.1, R, acc, 0.5, True, rowb0, S, pi)
            out['hg_conv/C%d/store/%s' % (C, prec)] = _sha(store)
            out['hg_conv/C%d/residual/%s' % (C, prec)] = _sha(res)
            out['hg_conv/C%d/accumulate/%s' % (C, prec)] = _sha(acc)
    # hg_upsample alone: 64 -> 32 channels, kernel 4, stride 2 (two phases with different tap bases)
    lens, S, H = [5, 1, 3], 2, 1
    rowb0, offs, P0 = _hg_plan(lens, H, dev)
    ci, co, ku, u = 64, 32, 4, 2
    g = torch.Generator().manual_seed(400)
    w = (torch.randn(ci, co, ku, generator=g) / (ci * ku / u) ** 0.5).to(dev)
    b = torch.randn(co, generator=g).to(dev)
    X = _image(lens, offs, P0, S, ci, 500, dev)
    wp, bp = pack_up(w, b, u, ci, co)
    for pi, prec in enumerate(PRECS):
        o = torch.full((P0 * S * u, co), 7.0, device=dev)
        nv.hg_upsample(X, wp, bp, ku, u, 0.1, o, rowb0, S, pi)
        out['hg_upsample/64_32_4_2/' + prec] = _sha(o)
    return out


def digests_vocos():
    """{'<entry>/<precision>': sha256}; needs cuda:0 and ``tacotron2_amd`` / tests/vocos_ref.py importable."""
    import torch
    import vocos_ref as vr
    from tacotron2_amd import native as nv
    from tacotron2_amd.vocos import Vocos, load_vocos
    dev = torch.device("cuda", 0)
    out = {}
    for name in ('small', 'odd'):                       # test_ragged_equals_alone_bitwise: D = 64 and 96
        ref = vr.make_ref(name, 0)
        c = ref.config
        voc = load_vocos(ref.state_dict(), hop_length=c['hop_length'], padding=c['padding']).to(dev).eval()
        mel = vr.make_mel(3, 40, 2, c['n_mel_channels']).to(dev)
        for prec in PRECS:
            voc.precision = prec
            out['%s/infer/%s' % (name, prec)] = _sha(voc.infer(mel))
            out['%s/infer_ragged/%s' % (name, prec)] = _sha(voc.infer(mel, lengths=[1, 7, 40]))
    # vc_linear alone, the three epilogues at every (D, I) of the test's DI: BN = 64, 32 and 128
    lens = [3, 1, 140]
    rowb0, _, _, offs, P = Vocos(**vr.CONFIGS['small']).packed_plan(lens)
    rowb0 = rowb0.to(dev)
    for i, (D, I) in enumerate([(64, 192), (96, 160), (512, 1536)]):
        g = torch.Generator().manual_seed(30 + i)
        w1, b1 = (torch.randn(I, D, generator=g) / D ** 0.5).to(dev), (0.1 * torch.randn(I, generator=g)).to(dev)
        w2, b2 = (torch.randn(D, I, generator=g) / I ** 0.5).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev)
        gamma = (0.5 * torch.randn(D, generator=g)).to(dev)
        X = _image(lens, offs, P, 1, D, 40 + i, dev)
        R = _image(lens, offs, P, 1, D, 50 + i, dev)
        for pi, prec in enumerate(PRECS):
            h = torch.full((P, I), 7.0, device=dev)
            nv.vc_linear(X, w1, b1, 'gelu', None, None, h, rowb0, pi)
            y = R.clone()
            nv.vc_linear(h, w2, b2, 'residual', gamma, y, y, rowb0, pi)
            plain = torch.full((P, D), 7.0, device=dev)
            nv.vc_linear(h, w2, None, None, None, None, plain, rowb0, pi)
            out['vc_linear/D%d_I%d/gelu/%s' % (D, I, prec)] = _sha(h)
            out['vc_linear/D%d_I%d/residual/%s' % (D, I, prec)] = _sha(y)
            out['vc_linear/D%d_I%d/plain/%s' % (D, I, prec)] = _sha(plain)
    return out


if __name__ == "__main__":
    root = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else ROOT
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "vocoder_digests.json")
    root = os.path.abspath(root)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    d = {"hifigan": digests_hifigan(), "vocos": digests_vocos()}
    import tacotron2_amd
    from tacotron2_amd import native
    assert os.path.abspath(os.path.dirname(os.path.dirname(tacotron2_amd.__file__))) == root, tacotron2_amd.__file__
    d["_meta"] = {"source_sha1": native.library_sha1()}
    with open(dst, "w") as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(d, indent=1, sort_keys=True))
