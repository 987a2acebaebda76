"""Convert the wavs of a filelist to another sampling rate on the GPU.

    python -m tacotron2_amd.resample FILELIST --to RATE -o DIR [--batch N] [--out-filelist PATH]

Reads the wav named in the first ``|``-field of every line (mono 16-bit PCM at any rate), groups the files by source rate,
converts each group in ragged batches of N with ``audio.Resample``, clips to the 16-bit range and writes
``DIR/<stem>.wav`` at RATE.  A file already at RATE is rewritten unchanged.  The new filelist (default ``DIR/<name of
FILELIST>``) names the written wavs, every other field unchanged: what ``train``, ``waveglow_train`` and ``vocos_train`` read.
"""
import argparse
import os
import sys

import numpy as np
import torch


def _gpu_resample(batch, orig, new, lengths):
    """(B, T) float32 host samples -> ((B, T') float32 host samples, new lengths) through ``audio.resample``."""
    from .audio import resample
    y, new_lengths = resample(torch.from_numpy(batch).cuda(), orig, new, lengths=lengths)
    return y.cpu().numpy(), new_lengths


def convert(filelist, to, out_dir, batch=16, resample_fn=None, out_filelist=None):
    """The host logic of the tool.  ``resample_fn(batch (B, T) float32 numpy in integer units, orig, new, lengths)`` -> ((B, T')
    array, new lengths) is the converter (default: the GPU's); rows of a batch are zero beyond their lengths.  Returns the list
    of (written path, samples)."""
    from scipy.io.wavfile import read, write
    from .utils import load_filepaths_and_text
    to, batch = int(to), int(batch)
    if to < 1 or batch < 1:
        raise ValueError("resample: --to and --batch must be positive, got %d and %d" % (to, batch))
    fn = _gpu_resample if resample_fn is None else resample_fn
    rows = load_filepaths_and_text(filelist)
    os.makedirs(out_dir, exist_ok=True)
    by_rate, dsts = {}, []
    for i, fields in enumerate(rows):
        sr, data = read(fields[0])
        if data.ndim != 1 or data.dtype != np.int16 or data.shape[0] < 1:
            raise ValueError("%s: expected mono 16-bit PCM, got shape %s of %s" % (fields[0], data.shape, data.dtype))
        dst = os.path.join(out_dir, os.path.splitext(os.path.basename(fields[0]))[0] + ".wav")
        if dst in dsts:
            raise ValueError("%s: two files of the list would be written to %s" % (fields[0], dst))
        dsts.append(dst)
        by_rate.setdefault(int(sr), []).append((i, data))
    written = [None] * len(rows)
    for sr in sorted(by_rate):
        group = by_rate[sr]
        for s in range(0, len(group), batch):
            part = group[s:s + batch]
            lengths = [d.shape[0] for _, d in part]
            if sr == to:
                outs, new_lengths = [d for _, d in part], lengths
            else:
                buf = np.zeros((len(part), max(lengths)), np.float32)
                for b, (_, d) in enumerate(part):
                    buf[b, :d.shape[0]] = d
                outs, new_lengths = fn(buf, sr, to, lengths)
            for b, (i, _) in enumerate(part):
                pcm = np.asarray(outs[b][:new_lengths[b]])
                if pcm.dtype != np.int16:
                    pcm = np.clip(np.rint(pcm), -32768, 32767).astype(np.int16)
                write(dsts[i], to, pcm)
                written[i] = (dsts[i], int(new_lengths[b]))
    out_filelist = out_filelist or os.path.join(out_dir, os.path.basename(filelist))
    with open(out_filelist, 'w', encoding='utf-8') as fh:
        fh.write('\n'.join('|'.join([dsts[i]] + fields[1:]) for i, fields in enumerate(rows)) + '\n')
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tacotron2_amd.resample", description=__doc__.split("\n\n")[0])
    ap.add_argument("filelist", help="path|text lines; the first field names a mono 16-bit wav")
    ap.add_argument("--to", type=int, required=True, metavar="RATE", help="the sampling rate to convert to")
    ap.add_argument("-o", "--out-dir", required=True)
    ap.add_argument("--batch", type=int, default=16, help="utterances per ragged batch (default 16)")
    ap.add_argument("--out-filelist", default=None, help="default: DIR/<name of FILELIST>")
    args = ap.parse_args(argv)
    for dst, T in convert(args.filelist, args.to, args.out_dir, args.batch, out_filelist=args.out_filelist):
        print(dst, T, "samples")
    return 0


if __name__ == "__main__":
    sys.exit(main())
