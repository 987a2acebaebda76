"""Score recordings under a WaveGlow checkpoint on the GPU: the negative log-likelihood in nats per sample.

    python -m tacotron2_amd.waveglow_score WAV [WAV ...] --waveglow CKPT [--sigma 1.0] [--precision fp32|bf16x3|bf16]
                                           [--hparams name=value,...] [--resample]

Every wav (16-bit PCM at ``hparams.sampling_rate``; at any rate with ``--resample``, converted by ``audio.Resample``) is scaled by ``max_wav_value``, turned into log-mels by
``TacotronSTFT.mel_spectrogram`` and trimmed to a multiple of the model's ``n_group``; all of them run as one ragged
batch through ``WaveGlow.nll`` (what the validation loop of NVIDIA's train.py computes with ``WaveGlowLoss``, per
utterance).  Prints one line per file (path, samples, nats per sample) and the length-weighted mean.
"""
import argparse
import sys

import torch


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tacotron2_amd.waveglow_score", description=__doc__.split("\n\n")[0])
    ap.add_argument("wavs", nargs="+", help="wav files at hparams.sampling_rate")
    ap.add_argument("--waveglow", required=True, metavar="CKPT", help="the WaveGlow checkpoint to score")
    ap.add_argument("--sigma", type=float, default=1.0, help="the sigma of WaveGlowLoss (default 1.0)")
    ap.add_argument("--precision", choices=("fp32", "bf16x3", "bf16"), default="fp32")
    ap.add_argument("--hparams", default="", help="comma-separated name=value overrides")
    ap.add_argument("--resample", action="store_true",
                    help="convert a wav at another rate to hparams.sampling_rate on the GPU instead of refusing it")
    args = ap.parse_args(argv)
    from .audio import TacotronSTFT, resample
    from .hparams import create_hparams
    from .utils import load_wav_to_torch
    from .waveglow import HOP, load_waveglow
    hp = create_hparams(args.hparams)
    if hp.hop_length != HOP:
        raise SystemExit("hop_length %d: WaveGlow upsamples by %d samples per mel frame" % (hp.hop_length, HOP))
    wg = load_waveglow(args.waveglow).cuda().eval()
    wg.precision = args.precision
    stft = TacotronSTFT(hp.filter_length, hp.hop_length, hp.win_length, hp.n_mel_channels, hp.sampling_rate,
                        hp.mel_fmin, hp.mel_fmax).cuda()
    G = wg.n_group
    signals, mels = [], []
    for p in args.wavs:
        x, sr = load_wav_to_torch(p)
        if sr != hp.sampling_rate and not args.resample:
            raise SystemExit("%s: sampling rate %d, expected %d" % (p, sr, hp.sampling_rate))
        if x.dim() != 1 or x.numel() < G:
            raise SystemExit("%s: expected mono audio of at least %d samples, got shape %s" % (p, G, tuple(x.shape)))
        x = x / hp.max_wav_value
        if sr != hp.sampling_rate:
            x = resample(x.cuda(), sr, hp.sampling_rate).clamp_(-1.0, 1.0).cpu()
            if x.numel() < G:
                raise SystemExit("%s: %d samples at %d Hz, at least %d are needed" % (p, x.numel(), hp.sampling_rate, G))
        x = x[:x.numel() // G * G]
        signals.append(x)
        mels.append(stft.mel_spectrogram(x.unsqueeze(0))[0])           # each file alone: its own reflected edges
    lengths = [x.numel() for x in signals]
    audio = torch.zeros(len(signals), max(lengths))
    mel = torch.zeros(len(signals), hp.n_mel_channels, max(m.shape[1] for m in mels), device=mels[0].device)
    for b, (x, m) in enumerate(zip(signals, mels)):
        audio[b, :x.numel()] = x
        mel[b, :, :m.shape[1]] = m
    nll = wg.nll(mel, audio.cuda(), sigma=args.sigma, lengths=lengths).cpu().tolist()
    for p, n, v in zip(args.wavs, lengths, nll):
        print("%s %d samples %.6f nats/sample" % (p, n, v))
    print("mean %.6f nats/sample over %d samples" % (sum(n * v for n, v in zip(lengths, nll)) / sum(lengths), sum(lengths)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
