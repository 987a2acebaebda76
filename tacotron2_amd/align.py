"""Per-token durations of a data set under a trained Tacotron 2, by forced alignment on the GPU
(``alignment.attention_durations``, csrc/align.hip).

    python -m tacotron2_amd.align --checkpoint CKPT --filelist FILE -o DIR [--hparams name=value,...] [--batch 16] [--posterior]

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
and summary are what they were."""
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


def align_checkpoint(checkpoint, filelist, hparams, out_dir, batch=16, with_posterior=False):
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
    rows, unalignable, post = [], [], []
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
        for k, (j, d, m) in enumerate(zip(keep, durs, metrics)):
            np.save(os.path.join(out_dir, names[j] + ".npy"), d.astype(np.int32))
            row = (names[j], ni[j], no[j]) + m
            line = "%s %d %d %.4f %.4f %.4f %d %d" % row
            if with_posterior:
                np.save(os.path.join(out_dir, names[j] + ".soft.npy"), more[0][k].astype(np.float32))
                line += " %.4f %.4f" % more[1][k]
                post.append(more[1][k])
            print(line)
            rows.append(row)
    return rows, summarise(rows, unalignable, post if with_posterior else None)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--checkpoint', required=True, help='a Tacotron 2 checkpoint')
    ap.add_argument('--filelist', required=True, help='the filelist (or synthetic:N) to align')
    ap.add_argument('-o', '--output', required=True, metavar='DIR', help='directory for NAME.npy and summary.json')
    ap.add_argument('--hparams', type=str, help='comma separated name=value pairs')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--posterior', action='store_true',
                    help='also write NAME.soft.npy (expected durations) and report log Z and the path\'s log posterior per frame')
    args = ap.parse_args(argv)
    if args.batch < 1:
        ap.error("--batch must be positive")
    from .hparams import create_hparams
    _, summary = align_checkpoint(args.checkpoint, args.filelist, create_hparams(args.hparams), args.output, args.batch, args.posterior)
    line = json.dumps(summary)
    print(line)
    with open(os.path.join(args.output, "summary.json"), 'w') as fh:
        fh.write(line + "\n")
    return summary


if __name__ == '__main__':
    main()
