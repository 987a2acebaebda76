"""Griffin-Lim vocoder without a GPU: the inverse basis and window envelope against the reference fixture, the argument
checks of the new entry points (validate-only), the packed frame space, and csrc/vocoder.hip's element kernels run on
the CPU through the host stand-in of tests/hip_emu (a separate library built into a temporary directory) -- the whole
Griffin-Lim loop of tacotron2_amd.audio with the GEMMs stood in by torch.matmul, against a float64 numpy restatement of
the reference's stft.py / audio_processing.py on a ragged L = 16 / hop = 4 batch."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import golden_util as gu
from tacotron2_amd import audio, native

EMU = os.path.join(gu.ROOT, "tests", "hip_emu")


def _golden(name):
    return torch.load(os.path.join(gu.GOLDEN_DIR, name), weights_only=False)


def _ulps(a, b):
    """distance in float32 ulps (of the larger magnitude)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / ulp.astype(np.float64)


def test_inverse_basis_and_window_sumsquare_match_reference_fixture():
    g = _golden("griffin_lim_basis.pt")
    ib64 = audio.inverse_basis(64, 16, 48)
    assert ib64.shape == (66, 64) and ib64.dtype == np.float32
    assert _ulps(ib64, g["ib64"].numpy()).max() <= 2
    ib = audio.inverse_basis(1024, 256, 1024)
    assert ib.shape == (1026, 1024)
    # pinv's last bits follow the LAPACK build and its thread split, so the digest is informative only: every 16th
    # element within 2 ulp and the norm are the check
    assert _ulps(ib.reshape(-1)[::16], g["ib1024_every16"].numpy()).max() <= 2
    assert abs(np.linalg.norm(ib.astype(np.float64)) - g["ib1024_norm"]) <= 1e-6 * g["ib1024_norm"]
    assert audio.inverse_basis(1024, 256, 1024) is ib                     # cached per geometry
    wss = audio.window_sumsquare('hann', 8, hop_length=256, win_length=1024, n_fft=1024)
    assert wss.dtype == np.float32 and np.array_equal(wss, g["wss1024_8"].numpy())


def test_tacotron_stft_does_not_build_the_inverse_basis():
    before = set(audio._INVERSE_BASES)
    st = audio.TacotronSTFT(filter_length=512, hop_length=128, win_length=512)
    assert set(audio._INVERSE_BASES) == before
    names = {k for k, _ in st.named_buffers()}
    assert not any("inverse" in k for k in names), names


def test_packed_rows():
    from tacotron2_amd.synth import synth_lengths
    _, to = synth_lengths(64, 1234)
    assert audio.packed_rows(to, 1024, 256) == int(to.sum()) + 3 * 64 == 36681
    for L, hop, lens in ((1024, 256, [870]), (16, 4, [5, 9, 4]), (800, 200, [7, 3]), (1000, 300, [4, 6]),
                         (64, 16, list(range(5, 30)))):
        c = -(-L // hop)
        want = sum(n + c - 1 for n in lens)
        assert audio.packed_rows(lens, L, hop) == want
    native.load()
    assert native.gl_packed_rows(to, 1024, 256) == 36681
    assert native.gl_packed_rows([5, 9, 4], 1000, 300) == audio.packed_rows([5, 9, 4], 1000, 300)
    assert native.gl_packed_rows([0, 4], 16, 4) == -1


@contextlib.contextmanager
def _validate_only():
    native.set_validate_only(True)
    try:
        yield
    finally:
        native.set_validate_only(False)


def _err(fn, *args, match):
    with pytest.raises(native.NativeError, match=match):
        fn(*args)


def test_entry_points_reject_bad_arguments(native_lib):
    L, hop, F, Fp = 16, 4, 9, 16
    lens = [5, 9, 4]
    R = audio.packed_rows(lens, L, hop)
    B = len(lens)
    plan = torch.zeros(2 * B + 1 + R, dtype=torch.int32)
    frames = torch.zeros(R, L)
    wsq = torch.ones(L, dtype=torch.float64)
    padded = torch.zeros(R * hop + L)
    spec = torch.zeros(R, 2 * Fp)
    S = torch.zeros(R, Fp)
    rec = torch.zeros(R, 2 * Fp)
    mag = torch.zeros(B, F, 9)
    with _validate_only():
        # the valid calls pass
        native.gl_overlap_add(frames, wsq, plan, lens, R, L, hop, 4.0, padded, 0)
        native.gl_overlap_add(frames, wsq, plan, lens, R, L, hop, 4.0, torch.zeros(B, 32), 1)
        native.gl_project(spec, S, plan, lens, R, L, hop, F, Fp, rec)
        native.gl_rect(mag, mag, plan, lens, R, L, hop, F, Fp, S, rec)
        native.stft_polar(spec[:12], 3, 4, F, torch.zeros(3, F, 4), torch.zeros(3, F, 4))
        native.mel_decompress(torch.zeros(2, 80, 7), torch.zeros(14, 80), [7, 3], torch.zeros(2, dtype=torch.int32))
        lib = native.load()
        ints = native._host_ints(lens)
        nul = None
        # null operands
        _err(native._check, lib.t2amd_gl_overlap_add_f32(nul, L, native.ptr(wsq, torch.float64), native.ptr(plan, torch.int32),
                                                          ints, B, R, L, hop, 4.0, native.ptr(padded), 0, padded.numel(), 0,
                                                          nul), "x", match="null operand")
        _err(native._check, lib.t2amd_gl_project_f32(native.ptr(spec), 2 * Fp, nul, Fp, native.ptr(plan, torch.int32), ints,
                                                      B, R, L, hop, F, Fp, native.ptr(rec), 2 * Fp, nul), "x",
             match="null operand")
        _err(native._check, lib.t2amd_gl_rect_f32(native.ptr(mag), nul, 9, nul, ints, B, R, L, hop, F, Fp, native.ptr(S), Fp,
                                                   native.ptr(rec), 2 * Fp, nul), "x", match="null operand")
        _err(native._check, lib.t2amd_stft_polar_f32(native.ptr(spec), 2 * Fp, 3, 4, F, nul, nul, nul), "x",
             match="null operand")
        _err(native._check, lib.t2amd_mel_decompress_f32(nul, 2, 80, 7, nul, nul, native.ptr(S), 80, nul), "x",
             match="null operand")
        _err(native._check, lib.t2amd_gl_overlap_add_f32(native.ptr(frames), L, native.ptr(wsq, torch.float64),
                                                          native.ptr(plan, torch.int32), nul, B, R, L, hop, 4.0,
                                                          native.ptr(padded), 0, padded.numel(), 0, nul), "x",
             match="null lengths")
        # rows too short
        _err(native.gl_overlap_add, torch.zeros(R, L - 1), wsq, plan, lens, R, L, hop, 4.0, padded, 0, match="too short")
        _err(native.gl_overlap_add, frames, wsq, plan, lens, R, L, hop, 4.0, padded[:(R - 1) * hop + L - 1], 0,
             match="shorter than")
        _err(native.gl_project, torch.zeros(R, 2 * F - 2), S, plan, lens, R, L, hop, F, Fp, rec, match="too short")
        _err(native.gl_project, spec, S, plan, lens, R, L, hop, F, Fp, torch.zeros(R, 2 * Fp - 2), match="too short")
        _err(native.gl_rect, mag, mag, plan, lens, R, L, hop, F, Fp, torch.zeros(R, F - 1), rec, match="too short")
        _err(native.stft_polar, torch.zeros(12, 2 * F - 2), 3, 4, F, torch.zeros(3, F, 4), None, match="too short")
        _err(native.mel_decompress, torch.zeros(2, 80, 7), torch.zeros(14, 79), match="too short")
        # n_b under the reflect limit ((n - 1) * hop must exceed L / 2 = 8: 3 frames are too few)
        short = [5, 3, 4]
        Rs = audio.packed_rows(short, L, hop)
        _err(native.gl_overlap_add, frames[:Rs], wsq, plan, short, Rs, L, hop, 4.0, padded, 0, match="reflect")
        native.gl_overlap_add(frames[:Rs], wsq, plan, short, Rs, L, hop, 4.0, torch.zeros(B, 32), 1)   # no padding: fine
        # lengths that do not fit the buffers
        _err(native.gl_project, spec, S, plan, [5, 9, 5], R, L, hop, F, Fp, rec, match="pack into")
        _err(native.gl_rect, torch.zeros(B, F, 8), torch.zeros(B, F, 8), plan, lens, R, L, hop, F, Fp, S, rec,
             match="more frames")
        _err(native.gl_overlap_add, frames, wsq, plan, lens, R, L, hop, 4.0, torch.zeros(B, 31), 1, match="longer than")
        _err(native.mel_decompress, torch.zeros(2, 80, 7), torch.zeros(14, 80), [8, 3], torch.zeros(2, dtype=torch.int32),
             match="exceeds")
        _err(native.gl_overlap_add, frames, wsq, plan, lens, R, L, hop, 4.0, torch.zeros(B, 32), 2, match="mode")


# ---------------------------------------------------------------------------------------------------------------
# csrc/vocoder.hip on the host stand-in
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vocoder_emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vocoder_emu") / "libvocoder_emu.so")
    src = [os.path.join(gu.ROOT, "tacotron2_amd", "csrc", "vocoder.hip"), os.path.join(EMU, "emu_runtime.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g0", "-w", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           "-I", EMU, "-x", "c++"] + src + ["-o", out])
    emu = ctypes.CDLL(out)
    assert emu.t2amd_emulated() == 1
    for name, at in native._argtypes().items():
        if hasattr(emu, name):
            fn = getattr(emu, name)
            fn.argtypes, fn.restype = at, ctypes.c_int
    emu.t2amd_last_error.restype = ctypes.c_char_p
    emu.t2amd_gl_packed_rows.argtypes, emu.t2amd_gl_packed_rows.restype = [ctypes.c_void_p] + [ctypes.c_int] * 3, ctypes.c_longlong
    return emu


@contextlib.contextmanager
def _emulated(emu):
    saved = (native._lib, native._validate_only, native.gemm, native.transpose)

    def gemm_standin(Cm, A, B, act=0, fast=0, batch=1, strides=(0, 0, 0)):   # C[M,N] = act(A[M,K] . B[N,K]^T) per batch item
        for b in range(batch):
            a = torch.as_strided(A, A.shape, A.stride(), A.storage_offset() + b * strides[0])
            w = torch.as_strided(B, B.shape, B.stride(), B.storage_offset() + b * strides[1])
            c = torch.as_strided(Cm, Cm.shape, Cm.stride(), Cm.storage_offset() + b * strides[2])
            r = a.double() @ w.double().t()
            c.copy_(torch.relu(r) if act else r)

    def transpose_standin(dst, src, batch=1, sstride=0, dstride=0):
        for b in range(batch):
            s = torch.as_strided(src, src.shape, src.stride(), src.storage_offset() + b * sstride)
            d = torch.as_strided(dst, dst.shape, dst.stride(), dst.storage_offset() + b * dstride)
            d.copy_(s.t())

    native._lib, native._validate_only = emu, True           # CPU pointers allowed, kernels DO run (emulated)
    native.gemm, native.transpose = gemm_standin, transpose_standin
    try:
        yield
    finally:
        native._lib, native._validate_only, native.gemm, native.transpose = saved


# float64 restatement of the reference (stft.py:42-141, audio_processing.py:7-76) for one utterance
class _RefSTFT:
    def __init__(self, L, hop, win):
        from scipy.signal import get_window
        self.L, self.hop, self.F = L, hop, L // 2 + 1
        fb = np.fft.fft(np.eye(L))
        fb = np.vstack([np.real(fb[:self.F]), np.imag(fb[:self.F])])
        w = audio._pad_center(get_window('hann', win, fftbins=True), L)
        self.fb = fb * w
        self.ib = np.linalg.pinv(L / hop * fb).T * w
        self.wsq = audio._pad_center(get_window('hann', win, fftbins=True) ** 2, L)

    def transform(self, x):
        L, hop, F = self.L, self.hop, self.F
        xp = np.pad(x, (L // 2, L // 2), mode='reflect')
        n = len(x) // hop + 1
        frames = np.stack([xp[j * hop:j * hop + L] for j in range(n)])
        spec = frames @ self.fb.T
        re, im = spec[:, :F].T, spec[:, F:].T
        return np.sqrt(re ** 2 + im ** 2), np.arctan2(im, re)

    def inverse(self, mag, phase):
        L, hop = self.L, self.hop
        n = mag.shape[1]
        rec = np.concatenate([mag * np.cos(phase), mag * np.sin(phase)], 0)
        frames = rec.T @ self.ib
        out = np.zeros(L + hop * (n - 1))
        wss = np.zeros_like(out)
        for j in range(n):
            out[j * hop:j * hop + L] += frames[j]
            wss[j * hop:j * hop + L] += self.wsq
        nz = wss > np.finfo(np.float32).tiny
        out[nz] /= wss[nz]
        out *= float(L) / hop
        return out[L // 2:len(out) - L // 2]

    def griffin_lim(self, mag, angles, n_iters):
        x = self.inverse(mag, angles)
        for _ in range(n_iters):
            _, ph = self.transform(x)
            x = self.inverse(mag, ph)
        return x


def _ragged_case(seed=0):
    rs = np.random.RandomState(seed)
    L, hop, win = 16, 4, 12
    lens = [5, 9, 4]
    n = max(lens)
    mag = np.zeros((3, L // 2 + 1, n), np.float32)
    ang = (rs.rand(*mag.shape) * 2 * np.pi - np.pi).astype(np.float32)
    for b, nb in enumerate(lens):
        mag[b, :, :nb] = rs.rand(L // 2 + 1, nb) + 0.05
    mag[1, 3, 2] = 0.0                                     # a zero target bin
    return L, hop, win, lens, mag, ang


@pytest.mark.parametrize("n_iters", [0, 1, 3])
def test_emulated_griffin_lim_ragged_matches_float64_reference(vocoder_emu, n_iters):
    L, hop, win, lens, mag, ang = _ragged_case()
    ref = _RefSTFT(L, hop, win)
    stft = audio.STFT(L, hop, win)
    with _emulated(vocoder_emu):
        gl = audio._GriffinLim(stft, torch.from_numpy(mag), torch.from_numpy(ang), lens, 'fp32')
        out = gl.run(n_iters).numpy().copy()
        R, Fp, F = gl.R, gl.Fp, gl.F
        rec, plan = gl.rec.numpy(), gl.plan.numpy()
        padded = gl.padded.numpy() if gl.padded is not None else None
    assert out.shape == (3, (max(lens) - 1) * hop)
    for b, nb in enumerate(lens):
        want = ref.griffin_lim(mag[b, :, :nb].astype(np.float64), ang[b, :, :nb].astype(np.float64), n_iters)
        T = (nb - 1) * hop
        got = out[b, :T]
        assert np.abs(got - want).max() <= 1e-5 * (1 + np.abs(want).max()), (b, np.abs(got - want).max())
        assert not out[b, T:].any()
    # gap rows and pad columns of the complex rows are zero; the padded signal is zero outside each utterance's segment
    row0 = plan[:4]
    assert not rec[:, 2 * F:].any()
    for b, nb in enumerate(lens):
        assert not rec[row0[b] + nb:row0[b + 1]].any()
        if padded is not None:
            seg = (nb - 1) * hop + L
            assert not padded[row0[b] * hop + seg:row0[b + 1] * hop].any()
            # the padded segment is the reflect-padded signal of this utterance
            x = padded[row0[b] * hop + L // 2:row0[b] * hop + L // 2 + (nb - 1) * hop]
            assert np.array_equal(padded[row0[b] * hop:row0[b] * hop + seg], np.pad(x, (L // 2, L // 2), mode='reflect'))
    if padded is not None:
        assert not padded[R * hop:].any()


def test_emulated_overlap_add_envelope_is_the_reference_float32_window_sumsquare(vocoder_emu):
    """All-ones frames: the overlap-add divides the frame count by the envelope -- compare with the reference's float32
    window_sumsquare bit for bit (the kernel rebuilds it in the same arithmetic)."""
    L, hop, win, n = 16, 4, 12, 7
    lens = [n]
    R = audio.packed_rows(lens, L, hop)
    plan = torch.from_numpy(np.concatenate([[0, R], lens, np.zeros(R)]).astype(np.int32))
    wsq = torch.from_numpy(audio._squared_window('hann', win, L))
    out = torch.zeros(1, (n - 1) * hop)
    frames = torch.ones(R, L)
    with _emulated(vocoder_emu):
        native.gl_overlap_add(frames, wsq, plan, lens, R, L, hop, 1.0, out, 1)
    wss = audio.window_sumsquare('hann', n, hop_length=hop, win_length=win, n_fft=L)
    cnt = np.zeros(L + hop * (n - 1), np.float32)
    for j in range(n):
        cnt[j * hop:j * hop + L] += 1
    want = np.where(wss > np.finfo(np.float32).tiny, cnt / np.where(wss > 0, wss, 1), cnt)[L // 2:-(L // 2)]
    assert np.array_equal(out[0].numpy(), want.astype(np.float32))


def test_emulated_polar_transform_matches_float64_reference(vocoder_emu):
    L, hop, win = 16, 4, 12
    rs = np.random.RandomState(3)
    y = rs.uniform(-1, 1, (2, 37)).astype(np.float32)
    ref = _RefSTFT(L, hop, win)
    stft = audio.STFT(L, hop, win)

    def reflect_standin(yt, out, pad):
        T = yt.shape[1]
        out.zero_()
        out[:, :T + 2 * pad] = torch.from_numpy(np.pad(yt.numpy(), ((0, 0), (pad, pad)), mode='reflect'))

    saved = native.reflect_pad
    native.reflect_pad = reflect_standin
    try:
        with _emulated(vocoder_emu):
            mag, phase = stft.transform(torch.from_numpy(y))
    finally:
        native.reflect_pad = saved
    for b in range(2):
        m, p = ref.transform(y[b].astype(np.float64))
        assert mag.shape[1:] == m.shape
        assert np.abs(mag[b].numpy() - m).max() <= 1e-5 * m.max()
        sel = m > 1e-3 * m.max()
        dp = np.angle(np.exp(1j * (phase[b].numpy() - p)))
        assert np.abs(dp[sel]).max() <= 1e-4


def test_emulated_mel_decompress(vocoder_emu):
    rs = np.random.RandomState(4)
    mel = torch.from_numpy(rs.uniform(-8, 1, (2, 5, 6)).astype(np.float32))
    out = torch.full((12, 8), 7.0)
    with _emulated(vocoder_emu):
        native.mel_decompress(mel, out, [6, 4], torch.tensor([6, 4], dtype=torch.int32))
    want = np.zeros((2, 6, 8), np.float32)
    want[:, :, :5] = np.exp(mel.numpy().astype(np.float64)).transpose(0, 2, 1)
    want[1, 4:] = 0
    assert np.allclose(out.numpy().reshape(2, 6, 8), want, rtol=2e-7, atol=0)
