"""The data set of NVIDIA's WaveGlow ``mel2samp.py``: random fixed-length segments of recordings and their mels.

    ds = Mel2Samp('filelists/train_files.txt', segment_length=16000)     # one wav path per line, or 'synthetic:N'
    audio = ds.collate([ds[i] for i in idx])                             # (B, segment_length) float32 in [-1, 1], host
    mel = ds.batch_mels(audio)                                           # (B, 80, 63) on the GPU, one front-end call per batch

mel2samp.py's contract: the file list is shuffled once with ``seed``; an item is a random segment of ``segment_length``
samples of its recording (a shorter recording is zero-padded at the end), divided by 32768.  What is different: cropping
is host work, the mel of the segments is computed per batch on the GPU by ``audio.TacotronSTFT.mel_spectrogram`` (the
reference computes it per item on the CPU); frames at or past ceil(segment_length / hop_length) are dropped, as glow.py's
``forward`` never reads them (16000 samples: all 63 frames are kept); and the start of a segment is a function of (seed, epoch,
item), not of a global generator's state, so a resumed run sees the segments the interrupted one would have seen.
``'synthetic:N'`` stands for N seeded noise-plus-tones recordings of 1 to 10 s, generated on the fly (no disk), as
``synth.py`` does for Tacotron 2.
"""
import random

import numpy as np
import torch

from .utils import load_wav_to_torch

MAX_WAV_VALUE = 32768.0


def files_to_list(filename):
    """One path per line (mel2samp.py's ``files_to_list``)."""
    with open(filename, encoding='utf-8') as fh:
        return [line.rstrip() for line in fh if line.strip()]


class Mel2Samp(torch.utils.data.Dataset):
    def __init__(self, training_files, segment_length=16000, filter_length=1024, hop_length=256, win_length=1024,
                 sampling_rate=22050, mel_fmin=0.0, mel_fmax=8000.0, seed=1234):
        self.segment_length, self.sampling_rate, self.hop_length, self.seed = segment_length, sampling_rate, hop_length, seed
        self.stft_args = (filter_length, hop_length, win_length, 80, sampling_rate, mel_fmin, mel_fmax)
        self.epoch = 0
        self._stft = None
        rnd = random.Random(seed)
        if isinstance(training_files, str) and training_files.startswith('synthetic:'):
            n = int(training_files.split(':', 1)[1])
            rs = np.random.RandomState(seed)
            self.synthetic_lengths = [int(v) for v in rs.randint(sampling_rate, 10 * sampling_rate + 1, n)]
            self.audio_files = ['synthetic:%d' % i for i in range(n)]
        else:
            self.synthetic_lengths = None
            self.audio_files = files_to_list(training_files) if isinstance(training_files, str) else list(training_files)
        rnd.shuffle(self.audio_files)

    @property
    def n_frames(self):
        """Mel frames per segment that ``WaveGlow.forward`` can reach: ceil(segment_length / hop_length)."""
        return -(-self.segment_length // self.hop_length)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return len(self.audio_files)

    def _synthetic(self, index):
        """Recording ``index`` in the wav range: white noise under three tones, seeded by (seed, index)."""
        i = int(self.audio_files[index].split(':')[1])
        n = self.synthetic_lengths[i]
        rs = np.random.RandomState([self.seed & 0x7fffffff, i])
        t = np.arange(n, dtype=np.float64) / self.sampling_rate
        x = 0.05 * rs.randn(n)
        for f, a in zip(rs.uniform(80.0, 4000.0, 3), rs.uniform(0.05, 0.25, 3)):
            x += a * np.sin(2.0 * np.pi * f * t + rs.uniform(0.0, 2.0 * np.pi))
        return torch.from_numpy(np.clip(x * MAX_WAV_VALUE, -MAX_WAV_VALUE, MAX_WAV_VALUE - 1.0).astype(np.float32))

    def __getitem__(self, index):
        if self.synthetic_lengths is not None:
            audio = self._synthetic(index)
        else:
            audio, sr = load_wav_to_torch(self.audio_files[index])
            if sr != self.sampling_rate:
                raise ValueError("{} SR doesn't match target {} SR: the sampling rate of {}".format(
                    sr, self.sampling_rate, self.audio_files[index]))
            if audio.dim() != 1:
                raise ValueError("Mel2Samp: %s is not a mono recording" % self.audio_files[index])
        n = audio.size(0)
        if n >= self.segment_length:
            rs = np.random.RandomState([self.seed & 0x7fffffff, self.epoch, index])
            start = int(rs.randint(0, n - self.segment_length + 1))
            audio = audio[start:start + self.segment_length]
        else:
            audio = torch.nn.functional.pad(audio, (0, self.segment_length - n), 'constant')
        return (audio / MAX_WAV_VALUE).contiguous()

    @staticmethod
    def collate(items):
        """Segments -> (B, segment_length) float32 on the host."""
        return torch.stack(list(items), 0)

    def batch_mels(self, audio):
        """(B, segment_length) audio in [-1, 1] (host or device) -> (B, 80, n_frames) mels on the GPU: the whole batch
        through ``TacotronSTFT.mel_spectrogram`` in one call."""
        from .audio import TacotronSTFT
        if self._stft is None:
            self._stft = TacotronSTFT(*self.stft_args)
        if torch.cuda.is_available():
            audio = audio.cuda(non_blocking=True)
            self._stft = self._stft.to(audio.device)
        return self._stft.mel_spectrogram(audio)[:, :, :self.n_frames].contiguous()
