"""The launches of the audio front end and the audio losses, in order, under validate-only: the no-GPU statement of "the same
launches in the same order".  A recording proxy around the loaded library notes every ``t2amd_*`` entry point that takes a
stream (the ones that launch; size queries such as ``t2amd_mel_l1_rows_per_slot`` are not launches).  The expected lists were
recorded with this very file from the commit BEFORE audio.py's three STFT front ends, two spectral backward tails and their
small helpers became one each, and are compared element for element.  Shapes: the smallest of tests/audio_grad_ref.py (case C)
and tests/stft_loss_ref.py (case A)."""
import contextlib

import torch

import audio_grad_ref as ar
import stft_loss_ref as sr
from tacotron2_amd import audio, native

PAD, GEMM, MAG, LOGC = 't2amd_reflect_pad_f32', 't2amd_gemm_f32', 't2amd_stft_magnitude_f32', 't2amd_mel_log_compress_f32'
MEL_FWD = [PAD, GEMM, MAG, GEMM, LOGC]
MEL_BWD = ['t2amd_mel_log_bwd_f32', GEMM, 't2amd_stft_magnitude_bwd_f32', GEMM, 't2amd_stft_frames_fold_f32']
SPEC_BWD = ['t2amd_stft_loss_bwd_f32', GEMM, 't2amd_stft_frames_fold_f32']
GL_ITER = [GEMM, 't2amd_gl_overlap_add_f32', GEMM, 't2amd_gl_project_f32']
EXPECTED = {
    'mel_spectrogram': MEL_FWD + MEL_BWD,
    'mel_loss_ragged': MEL_FWD + ['t2amd_mel_l1_fwd_f32', 't2amd_wg_partial_sum_f32', LOGC, 't2amd_mel_l1_bwd_f32'] + MEL_BWD,
    'stft_loss_R3': [PAD, PAD, GEMM] * 3 + ['t2amd_stft_loss_fwd_f32'] * 3 + ['t2amd_stft_loss_finish_f64'] + SPEC_BWD * 3
    + ['t2amd_stft_loss_sum_f32'],
    'stft_loss_R1': [PAD, PAD, GEMM, 't2amd_stft_loss_fwd_f32', 't2amd_stft_loss_finish_f64'] + SPEC_BWD,
    'stft_transform': [PAD, GEMM, 't2amd_stft_polar_f32'],
    'griffin_lim_2': ['t2amd_gl_rect_f32'] + GL_ITER * 2 + [GEMM, 't2amd_gl_overlap_add_f32'],
}


class _Recorder:
    """The loaded library with every call of a ``t2amd_*`` function that takes a stream noted by name."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        at = getattr(fn, 'argtypes', None)
        if not name.startswith('t2amd_') or not at or at[-1] is not native.C.c_void_p:
            return fn

        def call(*a):
            self._calls.append(name)
            return fn(*a)
        return call


@contextlib.contextmanager
def _recording():
    calls, lib = [], native.load()
    native.set_validate_only(True)
    native._lib = _Recorder(lib, calls)
    try:
        yield calls
    finally:
        native._lib = lib
        native.set_validate_only(False)


def _sequences():
    geom, B, T = ar.CASES['C']
    n = T // geom['hop_length'] + 1
    y = ar.signal('C').float()
    got = {}
    with _recording() as calls:
        st = audio.TacotronSTFT(**geom).cpu()
        x = y.clone().requires_grad_(True)
        st.mel_spectrogram(x, check_range=False).sum().backward()
        got['mel_spectrogram'] = list(calls)
        del calls[:]
        x = y.clone().requires_grad_(True)
        audio.MelLoss(st)(x, torch.zeros(B, geom['n_mel_channels'], n), lengths=[n, 1, n // 2]).backward()
        got['mel_loss_ragged'] = list(calls)
        xs, ys = (s.float() for s in sr.signals('A'))
        for tag, res in (('stft_loss_R3', sr.RESOLUTIONS), ('stft_loss_R1', sr.RESOLUTIONS[1:2])):
            del calls[:]
            a = xs.clone().requires_grad_(True)
            audio.MultiResolutionSTFTLoss(res).cpu()(a, ys).backward()
            got[tag] = list(calls)
        del calls[:]
        mag, _ = st.stft_fn.transform(y)
        got['stft_transform'] = list(calls)
        del calls[:]
        audio.griffin_lim(mag[:2], st.stft_fn, n_iters=2, angles=torch.zeros(2, mag.shape[1], n), lengths=[n, 5])
        got['griffin_lim_2'] = list(calls)
    return got


def test_launch_sequences_are_those_of_the_commit_before(native_lib):
    got = _sequences()
    assert sorted(got) == sorted(EXPECTED)
    for name in sorted(EXPECTED):
        assert got[name] == EXPECTED[name], name
