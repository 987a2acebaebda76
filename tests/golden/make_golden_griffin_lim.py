"""Golden fixtures of the Griffin-Lim vocoder (STFT phase, inverse STFT, griffin_lim).

    python tests/golden/make_golden_griffin_lim.py   # writes tests/golden/griffin_lim_demo.pt, griffin_lim_basis.pt

Runs only in the build container.  Executes the UNMODIFIED reference stft.py / audio_processing.py / layers.py on CPU
with librosa stubbed as make_golden_audio.py stubs it (``pad_center`` and ``mel`` from oracle/audio_oracle.py,
``tiny`` = np.finfo(float32).tiny, ``normalize(S, norm=None)`` = S).  Input: the two 9000-sample demo.wav slices
that tests/golden/audio_demo.pt already holds (key ``y``; not repeated here).

griffin_lim_demo.pt (signals):
  mag, phase       reference STFT.transform(y)                      (2, 513, 36)
  inverse          reference STFT.inverse(mag, phase)[:, 0]          (2, 8960)
  seed             np.random.seed(seed) before the reference's own angle draw (angles_sum: its float64 sum)
  gl_0, gl_1, gl_30  reference griffin_lim(mag, stft, n) from the seeded angles
  sc_0, sc_1, sc_30  spectral convergence ||mag - |STFT(x)| || / ||mag|| of those signals (reference transform)
  mel, mel_gl_30   the reference's mel_spectrogram(y) and griffin_lim(max(pinv(mel_basis) exp(mel), 0), 30) (same seed)
griffin_lim_basis.pt (tables; split off to keep each file well under 1 MB):
  ib64             the reference's inverse_basis for L = 64, hop = 16, win = 48, in full      (66, 64)
  ib1024_sha256, ib1024_norm, ib1024_every16   L = 1024, hop = 256: digest, float64 norm, flat[::16]
  wss1024_8        window_sumsquare('hann', 8, 256, 1024, 1024)
"""
import hashlib
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import audio_oracle as ao  # noqa: E402

REF = "/root/reference"
SEED = 4321


def import_reference():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    stub('librosa')
    stub('librosa.filters', mel=ao.librosa_mel)
    stub('librosa.util', pad_center=ao.pad_center, tiny=lambda x: np.finfo(np.float32).tiny,
         normalize=lambda S, norm=None: S)
    sys.modules['librosa'].filters = sys.modules['librosa.filters']
    sys.modules['librosa'].util = sys.modules['librosa.util']
    sys.path.insert(0, REF)
    import stft as ref_stft
    import audio_processing as ref_ap
    import layers as ref_layers
    sys.path.remove(REF)
    return ref_stft, ref_ap, ref_layers


def spectral_convergence(stft, mag, x):
    m, _ = stft.transform(x)
    return ((mag - m).double().flatten(1).norm(dim=1) / mag.double().flatten(1).norm(dim=1)).clone()


def main():
    ref_stft, ref_ap, ref_layers = import_reference()
    y = torch.load(os.path.join(HERE, "audio_demo.pt"), weights_only=False)["y"]
    assert tuple(y.shape) == (2, 9000)
    stft = ref_stft.STFT(1024, 256, 1024)
    with torch.no_grad():
        mag, phase = stft.transform(y)
        inv = stft.inverse(mag, phase)[:, 0]
        gl, sc = {}, {}
        for n in (0, 1, 30):
            np.random.seed(SEED)
            gl[n] = ref_ap.griffin_lim(mag, stft, n).clone()
            sc[n] = spectral_convergence(stft, mag, gl[n])
        np.random.seed(SEED)
        angles = np.angle(np.exp(2j * np.pi * np.random.rand(*mag.size()))).astype(np.float32)
        tac = ref_layers.TacotronSTFT()
        mel = tac.mel_spectrogram(y)
        pinv = torch.from_numpy(np.linalg.pinv(tac.mel_basis.double().numpy()).astype(np.float32))
        mel_mag = torch.clamp(torch.matmul(pinv, torch.exp(mel)), min=0.0)
        np.random.seed(SEED)
        mel_gl = ref_ap.griffin_lim(mel_mag, stft, 30).clone()
    demo = {"mag": mag.clone(), "phase": phase.clone(), "inverse": inv.clone(), "seed": SEED,
            "angles_sum": float(angles.astype(np.float64).sum()),
            "gl_0": gl[0], "gl_1": gl[1], "gl_30": gl[30], "sc_0": sc[0], "sc_1": sc[1], "sc_30": sc[30],
            "mel": mel.clone(), "mel_gl_30": mel_gl}
    torch.save(demo, os.path.join(HERE, "griffin_lim_demo.pt"))

    small = ref_stft.STFT(64, 16, 48)
    ib64 = small.inverse_basis[:, 0, :].clone()
    ib = stft.inverse_basis[:, 0, :].numpy()
    wss = ref_ap.window_sumsquare('hann', 8, hop_length=256, win_length=1024, n_fft=1024, dtype=np.float32)
    basis = {"ib64": ib64, "ib1024_sha256": hashlib.sha256(np.ascontiguousarray(ib).tobytes()).hexdigest(),
             "ib1024_norm": float(np.linalg.norm(ib.astype(np.float64))),
             "ib1024_every16": torch.from_numpy(ib.reshape(-1)[::16].copy()), "wss1024_8": torch.from_numpy(wss.copy())}
    torch.save(basis, os.path.join(HERE, "griffin_lim_basis.pt"))
    for name in ("griffin_lim_demo.pt", "griffin_lim_basis.pt"):
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")
    print("spectral convergence", {n: sc[n].tolist() for n in sc})


if __name__ == "__main__":
    main()
