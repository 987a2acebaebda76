"""sha256 of what the audio losses compute on an MI355X, per precision where a backward is involved: the mel front end and its
gradient, MelLoss, MultiResolutionSTFTLoss, STFT.transform, griffin_lim, the two d_spec row kernels alone, and the two clients of
the shared wave sum that no other fixture pins (Vocos' LayerNorm backward, WaveGlow's weight-norm fold).

    python tests/golden/make_golden_audio_digests.py [--root TREE] [--out tests/golden/audio_digests.json]

``--root`` selects the checkout whose ``tacotron2_amd`` is imported (default: this one), so the fixture can be written from the
commit BEFORE a change and compared with the commit after it, as tests/golden/make_golden_vocoder_digests.py does.
tests/test_zz18_audio_grad_gpu.py and tests/test_zz20_stft_loss_gpu.py recompute the digests: audio.py, csrc/audio_bwd.hip and
csrc/stft_loss.hip share their front end, their spectral backward and their device helpers (csrc/common.h), and a change to any
of them must not move a bit.  ``_meta.source_sha1`` is ``t2amd_source_sha1()`` of the library that wrote the fixture.

The shapes are the small cases of tests/audio_grad_ref.py (A: T = 513, both mirrors fold onto the same samples; C: B = 3, L = 512,
hop = 128, n_mel = 40, 2F no multiple of 4) and tests/stft_loss_ref.py (A: T = 65; Cr: ragged), with the loss's default eps, so
that bins on both sides of the clamp occur.  The row kernels alone run at F = 9, Kp = 64: Kp - 2F > F, the zero-tail loop runs
more than once per thread."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PRECS = ('fp32', 'bf16x3')
RAGGED = (12, 1, 6)                                  # frames of case C's three utterances


def _sha(*tensors):
    import numpy as np
    h = hashlib.sha256()
    for t in tensors:
        a = np.ascontiguousarray(t.detach().float().cpu().numpy())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def digests_mel():
    """{'<entry>[/<precision>]': sha256} of mel_spectrogram, MelLoss, STFT.transform, griffin_lim and the magnitude backward alone;
    needs cuda:0 and ``tacotron2_amd`` / tests/audio_grad_ref.py importable."""
    import torch
    import audio_grad_ref as ar
    from tacotron2_amd import native as nv
    from tacotron2_amd.audio import MelLoss, TacotronSTFT, griffin_lim
    dev = torch.device("cuda", 0)
    out = {}
    for name in ('A', 'C'):
        geom, B, T = ar.CASES[name]
        st = TacotronSTFT(**geom).to(dev)
        y = ar.signal(name).float().to(dev)
        r = ar.loss_weights((B, geom['n_mel_channels'], T // geom['hop_length'] + 1), 11).float().to(dev)
        out['mel_spectrogram/%s/out' % name] = _sha(st.mel_spectrogram(y))
        for prec in PRECS:
            x = y.clone().requires_grad_(True)
            (st.mel_spectrogram(x, check_range=False, precision=prec) * r).sum().backward()
            out['mel_spectrogram/%s/grad/%s' % (name, prec)] = _sha(x.grad)
    # st, y, B are case C's; a seeded target, so that no host arithmetic of another machine enters the digest
    target = (torch.randn(B, geom['n_mel_channels'], RAGGED[0], generator=torch.Generator().manual_seed(12)) - 2.0).to(dev)
    for tag, lens in (('full', None), ('ragged', list(RAGGED))):
        for prec in PRECS:
            x = y.clone().requires_grad_(True)
            loss = MelLoss(st)(x, target, lengths=lens, precision=prec)
            loss.backward()
            out['mel_loss/C/%s/%s' % (tag, prec)] = _sha(loss, x.grad)
    mag, phase = st.stft_fn.transform(y)
    out['stft_transform/C'] = _sha(mag, phase)
    g = torch.Generator().manual_seed(41)
    angles = (2.0 * torch.rand(2, mag.shape[1], mag.shape[2], generator=g) - 1.0) * 3.0
    for prec in PRECS:
        out['griffin_lim/C/' + prec] = _sha(griffin_lim(mag[:2].contiguous(), st.stft_fn, n_iters=2, angles=angles, lengths=[12, 5],
                                                        precision=prec))
    rows, F, Kp = 5, 9, 64
    g = torch.Generator().manual_seed(43)
    spec = torch.randn(rows, 2 * F, generator=g)
    spec[2, 3] = spec[2, F + 3] = 0.0                                      # a bin of magnitude exactly 0
    d_mag = torch.randn(rows, 16, generator=g).to(dev)
    d_spec = torch.full((rows, Kp), 7.0, device=dev)
    nv.stft_magnitude_bwd(d_mag, spec.to(dev), d_spec, F)
    out['stft_magnitude_bwd/F9_Kp64'] = _sha(d_spec)
    return out


def digests_stft_loss():
    """{'<entry>/<precision>': sha256} of MultiResolutionSTFTLoss (value, last_terms, gradient) and its backward kernel alone."""
    import torch
    import stft_loss_ref as sr
    from tacotron2_amd import native as nv
    from tacotron2_amd.audio import MultiResolutionSTFTLoss
    dev = torch.device("cuda", 0)
    out = {}
    for tag, res in (('R3', sr.RESOLUTIONS), ('R1', sr.RESOLUTIONS[1:2])):
        ml = MultiResolutionSTFTLoss(res).to(dev)
        for name in ('A', 'Cr'):
            lens = sr.CASES[name][2]
            x, y = (s.float().to(dev) for s in sr.signals(name))
            for prec in PRECS:
                a = x.clone().requires_grad_(True)
                loss = ml(a, y, lengths=None if lens is None else list(lens), precision=prec)
                terms = ml.last_terms
                loss.backward()
                out['stft_loss/%s/%s/%s' % (tag, name, prec)] = _sha(loss, terms, a.grad)
    n, F, Kp = 5, 9, 64
    g = torch.Generator().manual_seed(47)
    sx, sy = (torch.randn(n, 2 * F, generator=g).to(dev) for _ in range(2))
    sx[1, 2] = sx[1, F + 2] = 0.0                                          # below eps
    cnt = torch.tensor([4], dtype=torch.int32, device=dev)                 # the last row is outside the mask
    coef, up = torch.tensor([0.3, 0.02], device=dev), torch.tensor([0.7], device=dev)
    d_spec = torch.full((n, Kp), 7.0, device=dev)
    nv.stft_loss_bwd(sx, sy, cnt, coef, up, n, F, 1e-7, d_spec)
    out['stft_loss_bwd/F9_Kp64'] = _sha(d_spec)
    return out


def digests_wave_sum_clients():
    """Vocos' LayerNorm backward (with and without the recomputed convolution, D = 64 and 96) and WaveGlow's weight-norm fold and
    its backward (rows per lane, scalar rows, 16-byte rows kept in registers and read again).  vocoder_digests.json pins
    vc_dwln_kernel through Vocos.infer; these two are pinned nowhere else."""
    import torch
    import vocos_ref as vr
    from tacotron2_amd import native as nv
    from tacotron2_amd.vocos import Vocos
    dev = torch.device("cuda", 0)
    out = {}
    lens = [3, 1, 40]
    rowb0, _, _, offs, P = Vocos(**vr.CONFIGS['small']).packed_plan(lens)
    rowb0 = rowb0.to(dev)
    for D in (64, 96):
        g = torch.Generator().manual_seed(50 + D)
        w, cb, lw = (torch.randn(7, D, generator=g) / 7 ** 0.5).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev), \
            (1.0 + 0.1 * torch.randn(D, generator=g)).to(dev)
        X, G = torch.zeros(P, D), torch.zeros(P, D)
        for o, k in zip(offs, lens):
            X[o:o + k], G[o:o + k] = torch.randn(k, D, generator=g), torch.randn(k, D, generator=g)
        X, G = X.to(dev), G.to(dev)
        for tag, args in (('conv', (w, cb)), ('plain', (None, None))):
            dz = torch.full((P, D), 7.0, device=dev)
            part = torch.full((nv.vc_bwd_slots(P) * 2 * D,), 7.0, device=dev)
            nv.vc_ln_bwd(X, args[0], args[1], lw, vr.LN_EPS, rowb0, G, dz, part)
            out['vc_ln_bwd/D%d/%s' % (D, tag)] = _sha(dz, part)
    g = torch.Generator().manual_seed(53)
    lines, off, goff, dwoff = [], 0, 0, 8
    for ln in (1, 3, 4, 7, 96, 768, 1536):
        rows = 70 if ln <= 4 else 3
        lines.append((off, goff, dwoff, rows, ln))
        off, dwoff, goff = -(-(off + rows * ln) // 4) * 4, -(-(dwoff + rows * ln) // 4) * 4 + 4, goff + rows
    v, dw = torch.randn(off, generator=g).to(dev), torch.randn(dwoff, generator=g).to(dev)
    gg = (0.5 + torch.rand(-(-goff // 4) * 4, generator=g)).to(dev)
    host, n_units = nv.wg_weight_norm_table(lines)
    table = host.to(dev)
    wt, norm, dg, dv = (torch.full_like(t, 7.0) for t in (v, gg, gg, v))
    nv.wg_weight_norm(table, host, n_units, v, gg, wt, norm)
    nv.wg_weight_norm_bwd(table, host, n_units, dw, v, gg, norm, dg, dv, 0.5)
    out['wg_weight_norm/fold'] = _sha(wt, norm)
    out['wg_weight_norm/bwd'] = _sha(dg, dv)
    return out


if __name__ == "__main__":
    root = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else ROOT
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "audio_digests.json")
    root = os.path.abspath(root)
    sys.path[:0] = [root, os.path.join(root, "tests")]
    d = {"mel": digests_mel(), "stft_loss": digests_stft_loss(), "wave_sum_clients": digests_wave_sum_clients()}
    import tacotron2_amd
    from tacotron2_amd import native
    assert os.path.abspath(os.path.dirname(os.path.dirname(tacotron2_amd.__file__))) == root, tacotron2_amd.__file__
    d["_meta"] = {"source_sha1": native.library_sha1()}
    with open(dst, "w") as fh:
        json.dump(d, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(d, indent=1, sort_keys=True))
