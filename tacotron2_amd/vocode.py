"""mel -> wav with Griffin-Lim, WaveGlow, a HiFi-GAN generator or Vocos on the GPU.

    python -m tacotron2_amd.vocode MEL.npy [MEL.npy ...] -o DIR [--iters N] [--precision fp32|bf16x3] [--seed S]
    python -m tacotron2_amd.vocode MEL.npy [...] -o DIR --waveglow CKPT [--sigma 0.666] [--denoise STRENGTH]
                                   [--precision fp32|bf16x3|bf16] [--seed S]
    python -m tacotron2_amd.vocode MEL.npy [...] -o DIR --hifigan CKPT [--precision fp32|bf16x3|bf16]
    python -m tacotron2_amd.vocode MEL.npy [...] -o DIR --vocos CKPT [--precision fp32|bf16x3|bf16]

Reads (n_mel, n) float32 log-mels (what ``precompute_mels`` writes) or (B, n_mel, n) batches (one wav per item,
``<stem>_<b>.wav``), vocodes them as one ragged batch (``TacotronSTFT.vocode``, or ``WaveGlow.infer`` and optionally
``Denoiser`` with ``--waveglow``, or ``hifigan.Generator.infer`` with ``--hifigan``, or ``vocos.Vocos.infer`` with ``--vocos``: 256 samples per mel frame) and writes ``DIR/<stem>.wav``: 16-bit PCM at
``hparams.sampling_rate``, the signal clipped to [-1, 1] and scaled by ``max_wav_value``.  ``--sampling-rate R`` converts the
vocoder's output to R Hz first (``audio.Resample``) and the header says R.
"""
import argparse
import os
import sys

import numpy as np
import torch


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tacotron2_amd.vocode", description=__doc__.split("\n\n")[0])
    ap.add_argument("mels", nargs="+", help="(n_mel, n) or (B, n_mel, n) float32 .npy log-mel files")
    ap.add_argument("-o", "--out-dir", required=True)
    ap.add_argument("--iters", type=int, default=30, help="Griffin-Lim iterations (default 30)")
    ap.add_argument("--precision", choices=("fp32", "bf16x3", "bf16"), default="fp32",
                    help="bf16 applies to WaveGlow, HiFi-GAN and Vocos only")
    ap.add_argument("--seed", type=int, default=None,
                    help="np.random.seed before the initial angles are drawn (torch.manual_seed with --waveglow)")
    ap.add_argument("--waveglow", default=None, metavar="CKPT", help="vocode with this WaveGlow checkpoint")
    ap.add_argument("--hifigan", default=None, metavar="CKPT",
                    help="vocode with this HiFi-GAN generator checkpoint ({'generator': state dict}, weight-normed or folded)")
    ap.add_argument("--vocos", default=None, metavar="CKPT",
                    help="vocode with this Vocos checkpoint (a state dict or {'state_dict': ...}; hop from hparams, padding 'same')")
    ap.add_argument("--sigma", type=float, default=None, help="WaveGlow noise scale (default 0.666)")
    ap.add_argument("--denoise", type=float, default=0.0, metavar="STRENGTH",
                    help="WaveGlow Denoiser strength (default 0 = off)")
    ap.add_argument("--hparams", default="", help="comma-separated name=value overrides")
    ap.add_argument("--sampling-rate", type=int, default=None, metavar="R",
                    help="convert the vocoder's output to R Hz on the GPU before the clip (default: hparams.sampling_rate)")
    args = ap.parse_args(argv)
    if args.hifigan:
        # the generator draws no noise, and Denoiser is built from a WaveGlow's bias response
        if args.waveglow:
            ap.error("--hifigan and --waveglow are two vocoders: give one")
        if args.sigma is not None:
            ap.error("--sigma is WaveGlow's noise scale: a HiFi-GAN generator draws no noise")
        if args.denoise > 0:
            ap.error("--denoise is WaveGlow's Denoiser (built from a WaveGlow's bias response): not available with --hifigan")
    if args.vocos:
        if args.waveglow or args.hifigan:
            ap.error("--vocos, --hifigan and --waveglow are three vocoders: give one")
        if args.sigma is not None:
            ap.error("--sigma is WaveGlow's noise scale: Vocos draws no noise")
        if args.denoise > 0:
            ap.error("--denoise is WaveGlow's Denoiser (built from a WaveGlow's bias response): not available with --vocos")
    sigma = 0.666 if args.sigma is None else args.sigma
    from .audio import TacotronSTFT
    from .hparams import create_hparams
    hp = create_hparams(args.hparams)
    mels, names = [], []
    for p in args.mels:
        m = np.load(p).astype(np.float32)
        stem = os.path.splitext(os.path.basename(p))[0]
        if m.ndim == 3 and m.shape[1] == hp.n_mel_channels:          # a (B, n_mel, n) batch: one wav per item
            mels += list(m)
            names += ["%s_%d" % (stem, b) for b in range(m.shape[0])]
        elif m.ndim == 2 and m.shape[0] == hp.n_mel_channels:
            mels.append(m)
            names.append(stem)
        else:
            raise SystemExit("%s: expected (%d, n) or (B, %d, n) log-mels, got shape %s"
                             % (p, hp.n_mel_channels, hp.n_mel_channels, m.shape))
    lengths = [m.shape[1] for m in mels]
    batch = np.zeros((len(mels), hp.n_mel_channels, max(lengths)), np.float32)
    for b, m in enumerate(mels):
        batch[b, :, :m.shape[1]] = m
    if args.waveglow:
        from .waveglow import Denoiser, load_waveglow
        wg = load_waveglow(args.waveglow).cuda().eval()
        wg.precision = args.precision
        if args.seed is not None:
            torch.manual_seed(args.seed)
        audio = wg.infer(torch.from_numpy(batch).cuda(), sigma=sigma, lengths=lengths)
        if args.denoise > 0:
            audio = Denoiser(wg)(audio, strength=args.denoise)[:, 0]
        wav = audio.float().cpu().numpy()
        n_samples = [256 * n for n in lengths]
    elif args.hifigan:
        from .hifigan import load_hifigan
        hg = load_hifigan(args.hifigan, precision=args.precision).cuda().eval()
        if hg.n_mel_channels != hp.n_mel_channels:
            raise SystemExit("%s: the generator takes %d mel channels, the mels have %d"
                             % (args.hifigan, hg.n_mel_channels, hp.n_mel_channels))
        wav = hg.infer(torch.from_numpy(batch).cuda(), lengths=lengths)[:, 0].float().cpu().numpy()
        n_samples = [hg.hop * n for n in lengths]
    elif args.vocos:
        from .vocos import load_vocos
        try:
            vc = load_vocos(args.vocos, precision=args.precision, hop_length=hp.hop_length)
        except ValueError as e:
            raise SystemExit("%s: with hop %d from hparams: %s" % (args.vocos, hp.hop_length, e))
        if vc.n_mel_channels != hp.n_mel_channels:
            raise SystemExit("%s: the model takes %d mel channels, the mels have %d"
                             % (args.vocos, vc.n_mel_channels, hp.n_mel_channels))
        vc = vc.cuda().eval()
        wav = vc.infer(torch.from_numpy(batch).cuda(), lengths=lengths)[:, 0].float().cpu().numpy()
        n_samples = [vc.samples(n) for n in lengths]
    else:
        stft = TacotronSTFT(hp.filter_length, hp.hop_length, hp.win_length, hp.n_mel_channels, hp.sampling_rate,
                            hp.mel_fmin, hp.mel_fmax)
        if args.seed is not None:
            np.random.seed(args.seed)
        wav = stft.vocode(torch.from_numpy(batch), lengths=lengths, n_iters=args.iters, precision=args.precision).cpu().numpy()
        n_samples = [(n - 1) * hp.hop_length for n in lengths]
    rate = hp.sampling_rate
    if args.sampling_rate is not None and args.sampling_rate != rate:
        if args.sampling_rate < 1:
            ap.error("--sampling-rate must be positive")
        if min(n_samples) < 1:
            raise SystemExit("--sampling-rate: an utterance of %d samples cannot be converted" % min(n_samples))
        from .audio import resample
        sig = torch.from_numpy(np.ascontiguousarray(wav[:, :max(n_samples)], dtype=np.float32)).cuda()
        sig, n_samples = resample(sig, rate, args.sampling_rate, lengths=n_samples)
        wav, rate = sig.cpu().numpy(), args.sampling_rate
    from scipy.io.wavfile import write
    os.makedirs(args.out_dir, exist_ok=True)
    for b, name in enumerate(names):
        T = n_samples[b]
        # [-1, 1] * max_wav_value, kept inside int16 (1.0 * 32768 would wrap)
        pcm = np.clip(np.clip(wav[b, :T], -1.0, 1.0) * hp.max_wav_value, -32768, 32767).astype(np.int16)
        dst = os.path.join(args.out_dir, name + ".wav")
        write(dst, rate, pcm)
        print(dst, T, "samples")
    return 0


if __name__ == "__main__":
    sys.exit(main())
