"""Per-token durations of a data set under a trained Tacotron 2, by forced alignment on the GPU
(``alignment.attention_durations``, csrc/align.hip).

    python -m tacotron2_amd.align --checkpoint CKPT --filelist FILE -o DIR [--hparams name=value,...] [--batch 16]

Builds the model and the data set the way ``evaluate.evaluate_checkpoint`` does, runs the teacher-forced
``model(model.parse_batch(batch))`` in eval mode under ``no_grad`` and takes the best monotonic path through the log of the
returned attention matrix.  Writes ``DIR/NAME.npy`` (int32 frames per token; the entries sum to the utterance's mel frames) per
utterance, prints one line per utterance (name, tokens, frames, focus, path mass, off-path share, backward steps, longest
duration: ``alignment.alignment_metrics``) and a final JSON line with their means, also written to ``DIR/summary.json``.  An
utterance with fewer frames than tokens has no monotonic path: it is listed as ``unalignable`` and skipped."""
import argparse
import json
import os

import numpy as np
import torch

from . import alignment


def summarise(rows, unalignable):
    """The JSON summary of [(name, tokens, frames) + the five metrics]."""
    out = {"count": len(rows)}
    for i, k in enumerate(alignment.METRIC_KEYS):
        out[k + "_mean"] = float(np.mean([r[3 + i] for r in rows])) if rows else None
    out["unalignable"] = list(unalignable)
    return out


def measure(alignments, input_lengths, output_lengths):
    """Durations, path and metrics of the alignable utterances of one batch of attention matrices (B, To, Ti) -> (indices of
    the alignable utterances, their durations (numpy int32 rows cut to their tokens), their metric tuples)."""
    ni, no = [int(v) for v in input_lengths], [int(v) for v in output_lengths]
    keep = [b for b in range(len(ni)) if 1 <= ni[b] <= no[b]]
    if not keep:
        return [], [], []
    A = alignments[keep].float()
    ki, ko = [ni[b] for b in keep], [no[b] for b in keep]
    dur, _, path = alignment.attention_durations(A, ki, ko, return_path=True)
    m = alignment.alignment_metrics(A, path, ki, ko)
    dur = dur.cpu().numpy()
    return keep, [dur[j, :ki[j]] for j in range(len(keep))], [tuple(float(m[k][j]) for k in alignment.METRIC_KEYS)
                                                               for j in range(len(keep))]


def align_checkpoint(checkpoint, filelist, hparams, out_dir, batch=16):
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
    rows, unalignable = [], []
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
        keep, durs, metrics = measure(outs[3], ni, no)
        for j in range(len(idx)):
            if j not in keep:
                print("unalignable: %s %d %d" % (names[j], ni[j], no[j]))
                unalignable.append(names[j])
        for j, d, m in zip(keep, durs, metrics):
            np.save(os.path.join(out_dir, names[j] + ".npy"), d.astype(np.int32))
            row = (names[j], ni[j], no[j]) + m
            print("%s %d %d %.4f %.4f %.4f %d %d" % row)
            rows.append(row)
    return rows, summarise(rows, unalignable)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--checkpoint', required=True, help='a Tacotron 2 checkpoint')
    ap.add_argument('--filelist', required=True, help='the filelist (or synthetic:N) to align')
    ap.add_argument('-o', '--output', required=True, metavar='DIR', help='directory for NAME.npy and summary.json')
    ap.add_argument('--hparams', type=str, help='comma separated name=value pairs')
    ap.add_argument('--batch', type=int, default=16)
    args = ap.parse_args(argv)
    if args.batch < 1:
        ap.error("--batch must be positive")
    from .hparams import create_hparams
    _, summary = align_checkpoint(args.checkpoint, args.filelist, create_hparams(args.hparams), args.output, args.batch)
    line = json.dumps(summary)
    print(line)
    with open(os.path.join(args.output, "summary.json"), 'w') as fh:
        fh.write(line + "\n")
    return summary


if __name__ == '__main__':
    main()
