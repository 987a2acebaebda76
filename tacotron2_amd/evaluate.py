"""Mel-cepstral distortion under dynamic time warping (MCD-DTW) of synthesised mels against recordings, on the GPU
(``audio.MelCepstralDistortion``, csrc/dtw.hip).

    python -m tacotron2_amd.evaluate --mels DIR_A DIR_B [--n-coef 13] [--batch 16] [-o FILE]
    python -m tacotron2_amd.evaluate --checkpoint CKPT --filelist FILE [--hparams name=value,...] [--batch 16] [--alignment [--posterior]] [-o FILE]
    python -m tacotron2_amd.evaluate --wavs DIR_A DIR_B [--f0-min 60] [--f0-max 800] [--f0-threshold 0.1] [-o FILE]

Directory mode pairs the ``.npy`` natural-log mels (n_mel, frames) of the two directories by file name; names present on one side
only are listed and skipped.  Checkpoint mode builds the model and the data set the way ``train.py`` does, decodes every batch
free-running (``model.inference(text, input_lengths)``) and scores ``mel_outputs_postnet[:, :, :last_inference_lengths]`` against
the data set's mels.  Both print one line per utterance (name, frames A, frames B, path steps, MCD dB) and a final JSON line:
count, mean, standard deviation, median, mean length ratio (A over B) and, in checkpoint mode, the decodes that ran into
``max_decoder_steps``.  ``-o`` writes the same JSON to a file.

Wav mode pairs the mono 16-bit ``.wav`` files of two directories by name (both at the default hparams' sampling rate), takes their
mels with ``TacotronSTFT`` at the default hparams, the MCD with its DTW path, ``audio.yin`` at the mel's hop and ``audio.f0_metrics``
along the path.  Its lines carry the five fields above and then F0 RMSE in cents, F0 correlation,
voicing-decision error, gross pitch error and the both-voiced steps; its summary gains the mean and median of the RMSE, the means
of the other three (pairs without voiced overlap left out) and the count of such pairs.

``--alignment`` (checkpoint mode) also takes the best monotonic path through the free-running decode's attention matrix
(``alignment.attention_durations``) and appends focus, path mass, off-path share, backward steps and longest
duration (``alignment.alignment_metrics``) to each line, their means and the count of decodes shorter than their text
(``unalignable``) to the summary.  ``--alignment --posterior`` also sums over all monotonic paths (``alignment.alignment_posterior``,
DESIGN.md section 19): each line gains ``log_z / frames`` and ``(score - log_z) / frames``, the log posterior per frame of the best
path, and the summary their means ``log_likelihood_per_frame_mean`` and ``path_log_posterior_per_frame_mean``.  Without the flags
every mode prints what it printed before."""
import argparse
import json
import os

import numpy as np
import torch

from . import audio


def pair_directories(dir_a, dir_b):
    """-> (sorted names in both, sorted names only in A, sorted names only in B) of the ``.npy`` files."""
    def names(d):
        return set(f for f in os.listdir(d) if f.endswith('.npy'))
    a, b = names(dir_a), names(dir_b)
    return sorted(a & b), sorted(a - b), sorted(b - a)


def score_batch(mcd, mels_a, mels_b, device):
    """Lists of (n_mel, frames) host mels -> [(frames A, frames B, steps, MCD dB)] of one ``MelCepstralDistortion`` call."""
    def pad(mels):
        n_mel, T = mels[0].shape[0], max(m.shape[1] for m in mels)
        out = torch.zeros(len(mels), n_mel, T, dtype=torch.float32)
        for i, m in enumerate(mels):
            if m.dim() != 2 or m.shape[0] != n_mel or m.shape[1] < 1:
                raise ValueError("expected (n_mel, frames) mels of one n_mel, got shape %s beside n_mel %d" % (tuple(m.shape), n_mel))
            out[i, :, :m.shape[1]] = m
        return out.to(device), [m.shape[1] for m in mels]
    a, la = pad(mels_a)
    b, lb = pad(mels_b)
    db = mcd(a, b, la, lb).cpu().tolist()
    steps = mcd.last["steps"].cpu().tolist()
    return list(zip(la, lb, steps, db))


def summarise(rows, extra=None):
    """The JSON summary of [(name, frames A, frames B, steps, dB)]."""
    db = np.array([r[4] for r in rows], dtype=np.float64)
    ratio = np.array([r[1] / r[2] for r in rows], dtype=np.float64)
    out = {"count": len(rows),
           "mcd_db_mean": float(db.mean()) if len(rows) else None,
           "mcd_db_std": float(db.std()) if len(rows) else None,
           "mcd_db_median": float(np.median(db)) if len(rows) else None,
           "length_ratio_mean": float(ratio.mean()) if len(rows) else None}
    out.update(extra or {})
    return out


def _report(rows):
    for name, fa, fb, steps, db in rows:
        print("%s %d %d %d %.4f" % (name, fa, fb, steps, db))


def evaluate_directories(dir_a, dir_b, n_coef=13, batch=16, device='cuda'):
    both, only_a, only_b = pair_directories(dir_a, dir_b)
    for side, names in (("A", only_a), ("B", only_b)):
        for n in names:
            print("unmatched (only in %s): %s" % (side, n))
    mcd = audio.MelCepstralDistortion(n_coef)
    rows = []
    for k in range(0, len(both), batch):
        names = both[k:k + batch]
        ma = [torch.from_numpy(np.load(os.path.join(dir_a, n)).astype(np.float32)) for n in names]
        mb = [torch.from_numpy(np.load(os.path.join(dir_b, n)).astype(np.float32)) for n in names]
        got = [(n,) + r for n, r in zip(names, score_batch(mcd, ma, mb, device))]
        _report(got)
        rows += got
    return rows, summarise(rows, {"unmatched": only_a + only_b})


def evaluate_checkpoint(checkpoint, filelist, hparams, n_coef=13, batch=16, alignment=False, posterior=False):
    from .data_utils import TextMelCollate, TextMelLoader
    from .train import _read_checkpoint, load_model
    model = load_model(hparams)
    model.load_state_dict(_read_checkpoint(checkpoint)['state_dict'])
    model.eval()
    data = TextMelLoader(filelist, hparams)
    collate = TextMelCollate(hparams.n_frames_per_step)
    device = next(model.parameters()).device
    mcd = audio.MelCepstralDistortion(n_coef)
    rows, hit_max, arows, unalignable, prows = [], 0, [], 0, []
    if alignment:
        from . import align
    for k in range(0, len(data), batch):
        idx = list(range(k, min(k + batch, len(data))))
        items = [data[i] for i in idx]
        # the collate sorts by text length, descending; the names follow it
        order = torch.sort(torch.LongTensor([it[0].numel() for it in items]), dim=0, descending=True)[1].tolist()
        text, input_lengths, mel, _, output_lengths = collate(items)
        outs = model.inference(text.to(device).long(), input_lengths.to(device).long())
        got_len = [int(v) for v in torch.as_tensor(model.last_inference_lengths).tolist()]
        hit_max += sum(1 for v in got_len if v >= hparams.max_decoder_steps)
        post = outs[1].float().cpu()
        ma = [post[b, :, :max(1, got_len[b])] for b in range(len(idx))]
        mb = [mel[b, :, :int(output_lengths[b])] for b in range(len(idx))]
        names = [os.path.basename(data.audiopaths_and_text[idx[j]][0]) for j in order]
        got = [(n,) + r for n, r in zip(names, score_batch(mcd, ma, mb, device))]
        if alignment:
            keep, _, metrics, *more = align.measure(outs[3], input_lengths.tolist(), [max(1, v) for v in got_len], posterior)
            found = dict(zip(keep, metrics))
            if posterior:
                prows += more[1]
                tail = dict(zip(keep, (" %.4f %.4f" % p for p in more[1])))
            unalignable += len(idx) - len(keep)
            arows += [(names[j], 0, 0) + found[j] for j in keep]
            for j, (name, fa, fb, steps, db) in enumerate(got):
                print("%s %d %d %d %.4f %s" % (name, fa, fb, steps, db,
                                               "%.4f %.4f %.4f %d %d" % found[j] + (tail[j] if posterior else "")
                                               if j in found else "unalignable"))
        else:
            _report(got)
        rows += got
    extra = {"hit_max_decoder_steps": hit_max}
    if alignment:
        extra.update(align.summarise(arows, [], prows if posterior else None))
        extra.pop("count")
        extra["unalignable"] = unalignable
    return rows, summarise(rows, extra)


F0_KEYS = ("f0_rmse_cents", "f0_corr", "vuv_error", "gross_pitch_error")


def read_wav(path, hparams):
    """A mono 16-bit wav at the hparams' sampling rate -> (T,) float32 samples in [-1, 1)."""
    from scipy.io.wavfile import read
    sr, data = read(path)
    if data.ndim != 1 or data.dtype != np.int16:
        raise ValueError("%s: expected a mono 16-bit wav, got %s samples of shape %s" % (path, data.dtype, data.shape))
    if sr != hparams.sampling_rate:
        raise ValueError("%s: sampling rate %d, expected %d" % (path, sr, hparams.sampling_rate))
    if data.shape[0] < 1:
        raise ValueError("%s: no samples" % path)
    return torch.from_numpy(data.astype(np.float32) / np.float32(hparams.max_wav_value))


def summarise_f0(rows):
    """The F0 keys of the summary from [(name, frames A, frames B, steps, dB, cents, corr, vuv, gpe, voiced steps)]: means leave
    out the pairs without a both-voiced step (and a correlation that is NaN for a constant track)."""
    def stat(col, fn):
        v = np.array([r[col] for r in rows], dtype=np.float64)
        v = v[np.isfinite(v)]
        return float(fn(v)) if v.size else None
    return {"f0_rmse_cents_mean": stat(5, np.mean), "f0_rmse_cents_median": stat(5, np.median), "f0_corr_mean": stat(6, np.mean),
            "vuv_error_mean": stat(7, np.mean), "gross_pitch_error_mean": stat(8, np.mean),
            "no_voiced_overlap": sum(1 for r in rows if r[9] == 0)}


def evaluate_wavs(dir_a, dir_b, n_coef=13, f0_min=60.0, f0_max=800.0, f0_threshold=0.1, device='cuda'):
    from .hparams import create_hparams
    hp = create_hparams()
    def names(d):
        return set(f for f in os.listdir(d) if f.endswith('.wav'))
    a, b = names(dir_a), names(dir_b)
    both, only_a, only_b = sorted(a & b), sorted(a - b), sorted(b - a)
    for side, ns in (("A", only_a), ("B", only_b)):
        for n in ns:
            print("unmatched (only in %s): %s" % (side, n))
    pairs = [(n, read_wav(os.path.join(dir_a, n), hp), read_wav(os.path.join(dir_b, n), hp)) for n in both]   # refusals first
    stft = audio.TacotronSTFT(hp.filter_length, hp.hop_length, hp.win_length, hp.n_mel_channels, hp.sampling_rate, hp.mel_fmin,
                              hp.mel_fmax)
    mcd = audio.MelCepstralDistortion(n_coef, return_path=True)
    rows = []
    for n, wa, wb in pairs:
        wa, wb = wa.to(device).unsqueeze(0), wb.to(device).unsqueeze(0)
        db = float(mcd(stft.mel_spectrogram(wa), stft.mel_spectrogram(wb)).cpu()[0])
        last = mcd.last
        fa, va, _ = audio.yin(wa, None, hp.sampling_rate, hop_length=hp.hop_length, fmin=f0_min, fmax=f0_max, threshold=f0_threshold)
        fb, vb, _ = audio.yin(wb, None, hp.sampling_rate, hop_length=hp.hop_length, fmin=f0_min, fmax=f0_max, threshold=f0_threshold)
        m = audio.f0_metrics(fa, va, fb, vb, path=last["path"], steps=last["steps"])
        row = (n, last["len_a"][0], last["len_b"][0], int(last["steps"].cpu()[0]), db) \
            + tuple(float(m[k].cpu()[0]) for k in F0_KEYS) + (int(m["voiced_steps"].cpu()[0]),)
        print("%s %d %d %d %.4f %.3f %.4f %.4f %.4f %d" % row)
        rows.append(row)
    extra = summarise_f0(rows)
    extra["unmatched"] = only_a + only_b
    return rows, summarise(rows, extra)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--mels', nargs=2, metavar=('DIR_A', 'DIR_B'), help='two directories of .npy log-mels paired by file name')
    ap.add_argument('--checkpoint', help='a Tacotron 2 checkpoint to decode free-running')
    ap.add_argument('--filelist', help='the filelist (or synthetic:N) whose mels the decodes are scored against')
    ap.add_argument('--hparams', type=str, help='comma separated name=value pairs')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--n-coef', type=int, default=13, help='cepstral coefficients c1 ... cK, 1 to 32')
    ap.add_argument('--device', default='cuda', help=argparse.SUPPRESS)
    ap.add_argument('-o', '--output', help='write the JSON summary here as well')
    ap.add_argument('--wavs', nargs=2, metavar=('DIR_A', 'DIR_B'), help='two directories of mono 16-bit .wav files paired by name')
    ap.add_argument('--f0-min', type=float, default=60.0, help='lowest F0 of --wavs, Hz')
    ap.add_argument('--f0-max', type=float, default=800.0, help='highest F0 of --wavs, Hz')
    ap.add_argument('--f0-threshold', type=float, default=0.1, help="YIN's threshold on d' for --wavs")
    ap.add_argument('--alignment', action='store_true', help='with --checkpoint: alignment metrics of the decode\'s attention')
    ap.add_argument('--posterior', action='store_true',
                    help='with --alignment: log Z and the best path\'s log posterior per frame, summed over all monotonic paths')
    args = ap.parse_args(argv)
    if args.wavs is not None and (args.mels is not None or args.checkpoint is not None):
        ap.error("give one of --mels DIR_A DIR_B, --wavs DIR_A DIR_B or --checkpoint CKPT --filelist FILE")
    if args.wavs is None and (args.mels is None) == (args.checkpoint is None):
        ap.error("give either --mels DIR_A DIR_B or --checkpoint CKPT --filelist FILE")
    if args.batch < 1:
        ap.error("--batch must be positive")
    if args.alignment and args.checkpoint is None:
        ap.error("--alignment needs --checkpoint CKPT --filelist FILE")
    if args.posterior and not args.alignment:
        ap.error("--posterior needs --checkpoint CKPT --filelist FILE --alignment")
    if args.wavs is not None:
        if not args.f0_min < args.f0_max:
            ap.error("--f0-min must be below --f0-max")
        _, summary = evaluate_wavs(args.wavs[0], args.wavs[1], args.n_coef, args.f0_min, args.f0_max, args.f0_threshold, args.device)
    elif args.mels is not None:
        _, summary = evaluate_directories(args.mels[0], args.mels[1], args.n_coef, args.batch, args.device)
    else:
        if not args.filelist:
            ap.error("--checkpoint needs --filelist")
        from .hparams import create_hparams
        _, summary = evaluate_checkpoint(args.checkpoint, args.filelist, create_hparams(args.hparams), args.n_coef, args.batch,
                                         args.alignment, args.posterior)
    line = json.dumps(summary)
    print(line)
    if args.output:
        with open(args.output, 'w') as fh:
            fh.write(line + "\n")
    return summary


if __name__ == '__main__':
    main()
