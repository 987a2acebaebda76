"""Per-token durations of a data set under a trained Tacotron 2, by forced alignment on the GPU
(``alignment.attention_durations``, csrc/align.hip).

    python -m tacotron2_amd.align --checkpoint CKPT --filelist FILE -o DIR [--hparams name=value,...] [--batch 16] [--posterior]
                                  [--token-features]

Builds the model and the data set the way ``evaluate.evaluate_checkpoint`` does, runs the teacher-forced
``model(model.parse_batch(batch))`` in eval mode under ``no_grad`` and takes the best monotonic path through the log of the
returned attention matrix.  Writes ``DIR/NAME.npy`` (int32 frames per token; the entries sum to the utterance's mel frames) per
utterance, prints one line per utterance (name, tokens, frames, focus, path mass, off-path share, backward steps, longest
duration: ``alignment.alignment_metrics``) and a final JSON line with their means, also written to ``DIR/summary.json``.  An
utterance with fewer frames than tokens has no monotonic path: it is listed as ``unalignable`` and skipped.

``--posterior`` also sums over all monotonic paths through the same log attention (``alignment.alignment_posterior``,
csrc/forward_sum.hip): it writes ``DIR/NAME.soft.npy`` (float32 expected frames per token) beside
``NAME.npy``, appends ``log_z / frames`` and ``(score - log_z) / frames`` to each utterance's line (the latter is the log posterior
per frame of the path whose durations were written, <= 0 up to rounding: near 0 means the hard durations can be trusted) and adds
their means, ``log_likelihood_per_frame_mean`` and ``path_log_posterior_per_frame_mean``, to the summary.  Without the flag output
and summary are what they were.

``--token-features`` also writes the per-token prosody targets of a duration-based acoustic model beside ``NAME.npy``
(``alignment.token_average``, csrc/regulate.hip): ``DIR/NAME.energy.npy`` (float32, the mean over each
token's frames of the frame energy, the L2 norm over the mel channels of exp(log-mel)) and, where the loader reads wavs (neither
``synthetic:`` nor ``load_mel_from_disk``), ``DIR/NAME.f0.npy`` (float32 Hz, the mean of ``audio.yin``'s track at the mel's hop
over each token's voiced frames, 0 for a token without one); otherwise it prints one line saying that pitch is skipped.  The
summary gains ``energy_mean`` (over all tokens) and, with pitch, ``f0_voiced_token_share``.  Without the flag output and summary
are what they were."""
import argparse
import json
import os

import numpy as np
import torch

from . import alignment


POSTERIOR_KEYS = ("log_likelihood_per_frame", "path_log_posterior_per_frame")


def summarise(rows, unalignable, posterior=None):
    """The JSON summary of [(name, tokens, frames) + the five metrics]; with ``posterior`` (one pair of ``POSTERIOR_KEYS`` values
    per row) also their means."""
    out = {"count": len(rows)}
    for i, k in enumerate(alignment.METRIC_KEYS):
        out[k + "_mean"] = float(np.mean([r[3 + i] for r in rows])) if rows else None
    out["unalignable"] = list(unalignable)
    if posterior is not None:
        for i, k in enumerate(POSTERIOR_KEYS):
            out[k + "_mean"] = float(np.mean([p[i] for p in posterior])) if posterior else None
    return out


def posterior(alignments, input_lengths, output_lengths, score, eps=1e-8):
    """Soft durations and the two per-frame figures of alignable attention matrices (B, To, Ti) whose best paths scored ``score``
    (B,): the sum over all monotonic paths through the scores ``attention_durations`` took -> (numpy float32 rows cut to their
    tokens, [(log_z / frames, (score - log_z) / frames)])."""
    ni, no = [int(v) for v in input_lengths], [int(v) for v in output_lengths]
    _, soft, log_z = alignment.alignment_posterior(torch.log(alignments.detach().float().clamp_min(eps)), no, ni)
    soft, log_z, score = soft.cpu().numpy(), log_z.double().cpu().numpy(), score.double().cpu().numpy()
    return ([soft[j, :ni[j]] for j in range(len(ni))],
            [(float(log_z[j]) / no[j], (float(score[j]) - float(log_z[j])) / no[j]) for j in range(len(ni))])


def measure(alignments, input_lengths, output_lengths, with_posterior=False):
    """Durations, path and metrics of the alignable utterances of one batch of attention matrices (B, To, Ti) -> (indices of
    the alignable utterances, their durations (numpy int32 rows cut to their tokens), their metric tuples), and with
    ``with_posterior`` also what ``posterior`` returns for them."""
    ni, no = [int(v) for v in input_lengths], [int(v) for v in output_lengths]
    keep = [b for b in range(len(ni)) if 1 <= ni[b] <= no[b]]
    if not keep:
        return ([], [], [], [], []) if with_posterior else ([], [], [])
    A = alignments[keep].float()
    ki, ko = [ni[b] for b in keep], [no[b] for b in keep]
    dur, score, path = alignment.attention_durations(A, ki, ko, return_path=True)
    m = alignment.alignment_metrics(A, path, ki, ko)
    dur = dur.cpu().numpy()
    out = (keep, [dur[j, :ki[j]] for j in range(len(keep))], [tuple(float(m[k][j]) for k in alignment.METRIC_KEYS)
                                                              for j in range(len(keep))])
    return out + posterior(A, ki, ko, score) if with_posterior else out


def token_features(mel, durations, wavs=None, hparams=None):
    """Per-token energy, and with ``wavs`` (one (samples,) float tensor in [-1, 1] per utterance) per-token F0, of a batch: ``mel``
    (B, n_mel, To) log-mel on the device, ``durations`` a list of int rows.  -> ([float32 energy rows], [float32 F0 rows] or
    None)."""
    from . import audio
    dev, ni = mel.device, [len(d) for d in durations]
    dmat = torch.zeros(len(ni), max(ni), dtype=torch.int32)
    for j, d in enumerate(durations):
        dmat[j, :ni[j]] = torch.from_numpy(np.asarray(d, dtype=np.int32))
    dmat = dmat.to(dev)
    energy = alignment.token_average(torch.exp(mel.float()).norm(dim=1).contiguous(), dmat, ni).cpu().numpy()
    pitch = None
    if wavs is not None:
        To, lens = mel.shape[2], [int(w.numel()) for w in wavs]
        y = torch.zeros(len(wavs), max(lens))
        for j, w in enumerate(wavs):
            y[j, :lens[j]] = w
        f0, voiced, _ = audio.yin(y.to(dev), lens, sr=hparams.sampling_rate, frame_length=hparams.win_length,
                                  hop_length=hparams.hop_length)
        f0, voiced = (torch.nn.functional.pad(t.float(), (0, max(To - t.shape[1], 0)))[:, :To].contiguous() for t in (f0, voiced))
        pitch = alignment.token_average(f0, dmat, ni, weights=voiced).cpu().numpy()
    rows = lambda a: [a[j, :ni[j]].astype(np.float32) for j in range(len(ni))]                        # noqa: E731
    return rows(energy), None if pitch is None else rows(pitch)


def align_checkpoint(checkpoint, filelist, hparams, out_dir, batch=16, with_posterior=False, with_features=False):
    from .data_utils import TextMelCollate, TextMelLoader
    from .train import _read_checkpoint, load_model
    if hparams.n_frames_per_step != 1:
        raise ValueError("align: n_frames_per_step must be 1, got %d" % hparams.n_frames_per_step)
    model = load_model(hparams)
    model.load_state_dict(_read_checkpoint(checkpoint)['state_dict'])
    model.eval()
    data = TextMelLoader(filelist, hparams)
    collate = TextMelCollate(hparams.n_frames_per_step)
    os.makedirs(out_dir, exist_ok=True)
    rows, unalignable, post, energies, pitches = [], [], [], [], []
    with_pitch = with_features and data.synthetic is None and not hparams.load_mel_from_disk
    if with_features and not with_pitch:
        print("token features: pitch is skipped, the loader reads no wavs (a synthetic: filelist or load_mel_from_disk)")
    for k in range(0, len(data), batch):
        idx = list(range(k, min(k + batch, len(data))))
        items = [data[i] for i in idx]
        # the collate sorts by text length, descending; the names follow it
        order = torch.sort(torch.LongTensor([it[0].numel() for it in items]), dim=0, descending=True)[1].tolist()
        names = [os.path.splitext(os.path.basename(data.audiopaths_and_text[idx[j]][0]))[0] for j in order]
        b = collate(items)
        with torch.no_grad():
            outs = model(model.parse_batch(b)[0])
        ni, no = b[1].tolist(), b[4].tolist()
        keep, durs, metrics, *more = measure(outs[3], ni, no, with_posterior)
        for j in range(len(idx)):
            if j not in keep:
                print("unalignable: %s %d %d" % (names[j], ni[j], no[j]))
                unalignable.append(names[j])
        if with_features and keep:
            wavs = None
            if with_pitch:
                from .utils import load_wav_to_torch
                wavs = [load_wav_to_torch(data.audiopaths_and_text[idx[order[j]]][0])[0] / hparams.max_wav_value for j in keep]
            energy, pitch = token_features(b[2][keep].to(outs[3].device), durs, wavs, hparams)
        for k, (j, d, m) in enumerate(zip(keep, durs, metrics)):
            np.save(os.path.join(out_dir, names[j] + ".npy"), d.astype(np.int32))
            if with_features:
                np.save(os.path.join(out_dir, names[j] + ".energy.npy"), energy[k])
                energies.append(energy[k])
                if with_pitch:
                    np.save(os.path.join(out_dir, names[j] + ".f0.npy"), pitch[k])
                    pitches.append(pitch[k])
            row = (names[j], ni[j], no[j]) + m
            line = "%s %d %d %.4f %.4f %.4f %d %d" % row
            if with_posterior:
                np.save(os.path.join(out_dir, names[j] + ".soft.npy"), more[0][k].astype(np.float32))
                line += " %.4f %.4f" % more[1][k]
                post.append(more[1][k])
            print(line)
            rows.append(row)
    summary = summarise(rows, unalignable, post if with_posterior else None)
    if with_features:
        summary["energy_mean"] = float(np.concatenate(energies).mean()) if energies else None
        if with_pitch:
            summary["f0_voiced_token_share"] = float((np.concatenate(pitches) > 0).mean()) if pitches else None
    return rows, summary


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--checkpoint', required=True, help='a Tacotron 2 checkpoint')
    ap.add_argument('--filelist', required=True, help='the filelist (or synthetic:N) to align')
    ap.add_argument('-o', '--output', required=True, metavar='DIR', help='directory for NAME.npy and summary.json')
    ap.add_argument('--hparams', type=str, help='comma separated name=value pairs')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--posterior', action='store_true',
                    help='also write NAME.soft.npy (expected durations) and report log Z and the path\'s log posterior per frame')
    ap.add_argument('--token-features', action='store_true',
                    help='also write NAME.energy.npy and, where the loader reads wavs, NAME.f0.npy (per-token means)')
    args = ap.parse_args(argv)
    if args.batch < 1:
        ap.error("--batch must be positive")
    from .hparams import create_hparams
    _, summary = align_checkpoint(args.checkpoint, args.filelist, create_hparams(args.hparams), args.output, args.batch, args.posterior,
                                 args.token_features)
    line = json.dumps(summary)
    print(line)
    with open(os.path.join(args.output, "summary.json"), 'w') as fh:
        fh.write(line + "\n")
    return summary


if __name__ == '__main__':
    main()
