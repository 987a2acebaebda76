"""The length regulator without a GPU: the float64 restatement (tests/regulate_ref.py) against torch.repeat_interleave and float64
autograd, csrc/regulate.hip itself run on the host stand-in through the cases the GPU file shares (tests/regulate_cases.py),
the refusals, and the C entries' argument checks."""
import contextlib
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import regulate_cases as rc
import regulate_ref as rr
from tacotron2_amd import alignment, native

CPU = torch.device("cpu")


# ---- the restatements ----------------------------------------------------------------------------------------------------------
def test_float64_restatement_equals_repeat_interleave_and_float64_autograd():
    assert rr.check_against_torch() == 4 + 16 + 64 + 36


def test_fma32_is_correctly_rounded():
    """Against exact rational arithmetic, on operands chosen so that the float64 sum is itself inexact."""
    from fractions import Fraction
    g = np.random.RandomState(1)
    a, b = g.randn(4000).astype(np.float32), g.randn(4000).astype(np.float32)
    c = g.randn(4000).astype(np.float32)
    c[::2] = (-(a[::2].astype(np.float64) * b[::2]) * (1 + g.randn(2000) * 2.0 ** -20)).astype(np.float32)       # cancellation
    got = rr.fma32(a, b, c)
    for i in range(4000):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                                       # float(Fraction) rounds once to float64; then bracket
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda r: (abs(Fraction(float(r)) - exact), int(np.float32(r).view(np.int32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i])


def test_the_float32_restatement_is_close_to_the_float64_one():
    d = rc.durations(65, 130, "zeros")
    u = rc.utterance(tuple(int(v) for v in d), 8, 130, "frac")
    assert (np.abs(u["dx32"] - u["dx64"]) <= rr.gamma(u["cnt"] - 1)[:, None] * u["dx_mag"]).all()
    assert (np.abs(u["p32"]["m"] - u["p64"]["m"]) <= rr.pool_allowed(u["p64"])).all()


# ---- csrc/regulate.hip on the host stand-in ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_regulate_emu", os.path.join(gu.ROOT, "tests", "hip_emu", "build_regulate_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("regulate_emu"))))
    assert lib.t2amd_emulated() == 1
    for name, at in native._argtypes().items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = at, ctypes.c_int
    lib.t2amd_last_error.restype = ctypes.c_char_p
    return lib


@contextlib.contextmanager
def _emulated(lib):
    saved = (native._lib, native._validate_only)
    native._lib, native._validate_only = lib, True            # CPU pointers allowed, kernels DO run (emulated)
    try:
        yield
    finally:
        native._lib, native._validate_only = saved


@pytest.mark.parametrize("which", range(len(rc.SHAPES)))
def test_emulated_shapes(emu, which):
    with _emulated(emu):
        rc.shape_case(which, CPU)


def test_emulated_limits_and_overflowing_sums(emu):
    with _emulated(emu):
        assert native.regulate_limits() == (alignment.MAX_CHANNELS, alignment.MAX_TOKENS, alignment.MAX_REGULATED_FRAMES) == (512, 1024, 65536)
        rc.overflowing_sums(CPU)


def test_emulated_ragged_batch_equals_each_utterance_alone(emu):
    with _emulated(emu):
        rc.ragged_equals_alone(CPU)


def test_emulated_many_short_utterances(emu):
    with _emulated(emu):
        rc.many_short(CPU)


def test_emulated_pooling_forms(emu):
    with _emulated(emu):
        rc.pooling_forms(CPU)


def test_emulated_round_trip_with_monotonic_align(emu):
    with _emulated(emu):
        rc.round_trip(CPU)


def test_emulated_planted_identity(emu):
    with _emulated(emu):
        rc.planted_identity(CPU)


def test_emulated_autograd(emu):
    with _emulated(emu):
        rc.autograd(CPU)


def test_refusals(emu):
    with _emulated(emu):                                                    # host tensors pass the device check here
        rc.refusals(CPU)


def test_host_tensors_are_refused():
    x, d = torch.zeros(1, 3, 2), torch.ones(1, 3, dtype=torch.int32)
    for call in (lambda: alignment.length_regulate(x, d), lambda: alignment.length_regulate(x, d, None, 4),
                 lambda: alignment.durations_to_path(d), lambda: alignment.token_average(torch.zeros(1, 3), d),
                 lambda: alignment.LengthRegulator()(x, d.float())):
        with pytest.raises(native.NativeError, match="no CPU path"):
            call()


# ---- the C entries' own checks -------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments(emu):
    buf = torch.zeros(1 << 18)                                              # the good calls run: zeros are durations of 0
    base = buf.data_ptr() // 16 * 16 + 16
    at = lambda i: ctypes.c_void_p(base + i * (1 << 16))                    # noqa: E731
    d, nl, path, tl, ends, x, y, dx, w = (at(i) for i in range(9))
    paths = lambda **kw: emu.t2amd_durations_to_path_i32(*[kw.get(n, v) for n, v in (             # noqa: E731
        ("d", d), ("bytes", 4), ("db", 8), ("nl", nl), ("B", 2), ("N", 8), ("T", 16), ("path", path), ("tl", tl), ("ends", ends),
        ("totals", None), ("stream", None))])
    assert paths() == 0 and paths(T=0, path=None) == 0 and paths(nl=None, ends=None, bytes=8) == 0
    for kw, word in ((dict(d=None), b"durations_to_path: null operand"), (dict(tl=None), b"null operand"), (dict(B=0), b"1 to 65535 utterances"),
                     (dict(N=0), b"at least 1 token"), (dict(N=1025), b"at most 1024 tokens"), (dict(T=-1), b"a frame count of at least 0"),
                     (dict(T=65537), b"at most 65536 frames"), (dict(bytes=2), b"int32 (4) or int64 (8)"), (dict(db=7), b"duration stride"),
                     (dict(path=d), b"must not overlap"), (dict(ends=d), b"must not overlap")):
        assert paths(**kw) != 0 and word in emu.t2amd_last_error(), word
    fwd = lambda **kw: emu.t2amd_length_regulate_f32(*[kw.get(n, v) for n, v in (                  # noqa: E731
        ("x", x), ("xb", 32), ("xn", 4), ("path", path), ("B", 2), ("N", 8), ("T", 16), ("C", 4), ("y", y), ("stream", None))])
    assert paths() == 0 and fwd() == 0 and fwd(x=ctypes.c_void_p(x.value + 4)) == 0
    for kw, word in ((dict(x=None), b"length_regulate: null operand"), (dict(C=513), b"1 to 512 channels"), (dict(C=0), b"1 to 512 channels"),
                     (dict(T=0), b"at least 1 frame"), (dict(xn=3), b"token strides"), (dict(xb=31), b"token strides"),
                     (dict(y=x), b"must not overlap")):
        assert fwd(**kw) != 0 and word in emu.t2amd_last_error(), word
    bwd = lambda **kw: emu.t2amd_length_regulate_bwd_f32(*[kw.get(n, v) for n, v in (              # noqa: E731
        ("dy", y), ("gb", 64), ("gt", 4), ("ends", ends), ("B", 2), ("N", 8), ("T", 16), ("C", 4), ("dx", dx), ("stream", None))])
    assert bwd() == 0
    for kw, word in ((dict(ends=None), b"length_regulate_bwd: null operand"), (dict(gt=3), b"gradient strides"), (dict(gb=63), b"gradient strides"),
                     (dict(N=1025), b"at most 1024 tokens"), (dict(dx=y), b"must not overlap")):
        assert bwd(**kw) != 0 and word in emu.t2amd_last_error(), word
    m, den = at(9), at(10)
    avg = lambda **kw: emu.t2amd_token_average_f32(*[kw.get(n, v) for n, v in (                    # noqa: E731
        ("v", y), ("vb", 64), ("vt", 4), ("w", w), ("wb", 16), ("ends", ends), ("B", 2), ("N", 8), ("T", 16), ("C", 4), ("m", m), ("den", den),
        ("num", None), ("stream", None))])
    assert avg() == 0 and avg(w=None, wb=0) == 0 and avg(num=at(11)) == 0
    for kw, word in ((dict(den=None), b"token_average: null operand"), (dict(vt=3), b"value strides"), (dict(wb=15), b"weight stride"),
                     (dict(T=65537), b"at most 65536 frames"), (dict(m=y), b"must not overlap"), (dict(num=m), b"must not overlap")):
        assert avg(**kw) != 0 and word in emu.t2amd_last_error(), word
    avb = lambda **kw: emu.t2amd_token_average_bwd_f32(*[kw.get(n, v) for n, v in (                # noqa: E731
        ("g", m), ("den", den), ("w", w), ("wb", 16), ("path", path), ("B", 2), ("N", 8), ("T", 16), ("C", 4), ("dv", dx), ("stream", None))])
    assert avb() == 0
    for kw, word in ((dict(path=None), b"token_average_bwd: null operand"), (dict(wb=15), b"weight stride"), (dict(C=513), b"1 to 512 channels"),
                     (dict(dv=m), b"must not overlap")):
        assert avb(**kw) != 0 and word in emu.t2amd_last_error(), word
    assert emu.t2amd_regulate_limits(None, None, None) != 0 and b"regulate_limits: null operand" in emu.t2amd_last_error()


def test_the_library_exports_the_entries_and_refuses_in_validate_only_form(native_lib):
    lib = native_lib
    p = ctypes.c_void_p(torch.zeros(1 << 12).data_ptr() // 16 * 16 + 16)
    q = ctypes.c_void_p(p.value + (1 << 13))
    native.set_validate_only(True)
    try:
        assert native.regulate_limits() == (512, 1024, 65536)
        assert lib.t2amd_durations_to_path_i32(p, 4, 8, None, 1, 8, 16, None, q, None, None, None) == 0
        assert lib.t2amd_durations_to_path_i32(p, 4, 8, None, 1, 8, 65537, None, q, None, None, None) != 0
        assert b"durations_to_path: at most 65536 frames" in lib.t2amd_last_error()
        assert lib.t2amd_length_regulate_f32(p, 32, 4, q, 1, 8, 16, 513, q, None) != 0 and b"1 to 512 channels" in lib.t2amd_last_error()
        assert lib.t2amd_length_regulate_bwd_f32(None, 64, 4, q, 1, 8, 16, 4, q, None) != 0 and b"null operand" in lib.t2amd_last_error()
        assert lib.t2amd_token_average_f32(p, 64, 3, None, 0, q, 1, 8, 16, 4, q, q, None, None) != 0 and b"value strides" in lib.t2amd_last_error()
        assert lib.t2amd_token_average_bwd_f32(p, p, None, 0, None, 1, 8, 16, 4, q, None) != 0 and b"null operand" in lib.t2amd_last_error()
    finally:
        native.set_validate_only(False)
