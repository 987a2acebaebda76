"""The sample-rate converter without a GPU: the float64 restatement (tests/resample_ref.py) against the dense formulation it
departs from and against an analytic sine, the structure of the compact tables, csrc/resample.hip itself run on the host stand-in
against the restatement and its autograd, the refusals, and the corpus tool's host logic."""
import contextlib
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import resample_ref as rr
from tacotron2_amd import audio, native
from tacotron2_amd import resample as tool

PAIRS = [(48000, 22050), (24000, 22050), (16000, 22050), (22050, 16000), (44100, 22050), (22050, 44100)]
SMALL = [(3, 2), (2, 3), (7, 5), (147, 160)]
MEMORY_RATIO = (1031, 1030)              # 1030 phases of 13 taps: beyond the 8192 floats of the table's LDS budget
RATIOS = [(3, 2), (2, 3), (7, 5), (320, 147), MEMORY_RATIO]


# ---- the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS + SMALL)
def test_restatement_equals_the_unclamped_dense_formulation(pair):
    a = rr.dense_table(*pair)
    b = rr.dense_table(*pair, zero_outside=False)
    print("\nFIGURE %s: max |zeroed - clamped| = %.3e" % (pair, (a - b).abs().max().item()))
    assert (a - b).abs().max().item() <= 1e-15
    x = rr.signal(2, 700, 11).double()
    assert (rr.resample(x, *pair) - rr.resample(x, *pair, table=b)).abs().max().item() <= 1e-15
    # the unfold-and-matmul statement of the same sums (what the GPU tests run): float64 rounding of another summation order
    assert (rr.resample(x, *pair) - rr.resample(x, *pair, lengths=[700, 700], conv=False)).abs().max().item() <= 1e-14


@pytest.mark.parametrize("pair", PAIRS)
def test_restatement_against_an_analytic_sine(pair):
    orig, new = pair
    f = 0.2 * min(orig, new)
    T = 4000
    x = torch.sin(2 * math.pi * f * torch.arange(T, dtype=torch.float64) / orig)[None, :]
    y = rr.resample(x, orig, new)[0]
    m = torch.arange(y.shape[0], dtype=torch.float64)
    want = torch.sin(2 * math.pi * f * m / new)
    edge = int(math.ceil(40 * new / min(orig, new)))                     # well inside: the filter spans about 6 periods of base
    err = (y - want)[edge:-edge].abs().max().item()
    print("\nFIGURE %s: sine at %.0f Hz, max abs error on interior samples %.3e" % (pair, f, err))
    assert err < 1e-3


def test_unfold_statement_of_the_mel_restatement():
    """The GPU suite's ``_logmel`` (frames times basis) is audio_grad_ref.logmel (strided conv1d) up to float64 rounding."""
    import audio_grad_ref as ar
    import test_zz21_resample_gpu as gpu_tests
    y = ar.signal('B')
    assert (gpu_tests._logmel(y, ar.DEFAULT) - ar.logmel(y, ar.DEFAULT)).abs().max().item() <= 1e-10


def test_restatement_adjoint_identity():
    for orig, new in RATIOS:
        x = rr.signal(2, 301, 5).double().requires_grad_(True)
        y = rr.resample(x, orig, new, lengths=[301, 77])
        g = torch.randn(y.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        (gx,) = torch.autograd.grad(y, x, g)
        lhs, rhs = (y * g).sum().item(), (x * gx).sum().item()
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), y.norm().item() * g.norm().item())
        assert not gx[1, 77:].any()


# ---- the tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", PAIRS + SMALL + [(320, 147), MEMORY_RATIO])
def test_compact_tables_reproduce_the_dense_table(pair):
    tb = audio.resample_tables(*pair)
    o, n, base, width = rr.geometry(*pair)
    assert (tb["o"], tb["n"], tb["width"]) == (o, n, width)
    dense = rr.dense_table(*pair).float().numpy()
    assert np.array_equal(tb["dense"], dense)                             # the package's own statement, bit for bit
    tab, first = tb["tab"], tb["first"]
    S, K = tab.shape[1], 2 * width + o
    assert S <= math.ceil(2 * 6 * o / base) and first.min() >= 0 and (first + S).max() <= K
    back = np.zeros_like(dense)
    for j in range(n):
        back[j, first[j]:first[j] + S] = tab[j]
    assert np.array_equal(back, dense)
    # the adjoint's table holds the same coefficients: d_x[Q o + r] reads output (Q n + bfirst[r] + s - wpad) = q n + j at tap
    # k = Q o + r + width - q o
    btab, bfirst = tb["btab"], tb["bfirst"]
    Sb = btab.shape[1]
    assert Sb <= math.ceil(2 * 6 * n / base) and bfirst.min() == 0 and (bfirst + Sb).max() == tb["Kd"]
    seen = np.zeros_like(dense)
    for r in range(o):
        for s in range(Sb):
            d = int(bfirst[r]) + s - tb["wpad"]
            c, j = d // n, d % n
            k = r + width - c * o
            if 0 <= k < K:
                assert btab[r, s] == dense[j, k]
                seen[j, k] = dense[j, k]
            else:
                assert btab[r, s] == 0.0
    assert np.array_equal(seen, dense)                                    # every non-zero tap is in the adjoint's table


def test_tap_counts_of_the_two_named_pairs():
    assert audio.resample_tables(48000, 22050)["tab"].shape == (147, 27)
    assert audio.resample_tables(16000, 22050)["tab"].shape[1] == 13


# ---- csrc/resample.hip on the host stand-in ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_resample_emu",
                                                  os.path.join(gu.ROOT, "tests", "hip_emu", "build_resample_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("resample_emu"))))
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


_TABLES = {}


def _tables(pair):
    if pair not in _TABLES:
        h = audio.resample_tables(*pair)
        _TABLES[pair] = dict((k, torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in h.items())
    return _TABLES[pair]


def _run(pair, x, g, lens):
    """Both launches on buffers wider than their rows, pre-filled with 7.0 -> (y, d_x) and the check of the margins."""
    tb = _tables(pair)
    B, T = x.shape
    Tout = rr.output_length(*pair, T)
    xb, yb = torch.full((B, T + 5), 7.0), torch.full((B, Tout + 3), 7.0)
    gb, db = torch.full((B, Tout + 3), 7.0), torch.full((B, T + 5), 7.0)
    xb[:, :T], gb[:, :Tout] = x, g
    lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32)
    native.resample_fwd(xb[:, :T], lens_t, yb[:, :Tout], tb["tab"], tb["first"], tb["o"], tb["n"], tb["width"])
    native.resample_bwd(gb[:, :Tout], lens_t, db[:, :T], tb["btab"], tb["bfirst"], tb["o"], tb["n"], tb["wpad"], tb["Kd"])
    assert (yb[:, Tout:] == 7.0).all() and (db[:, T:] == 7.0).all()
    assert torch.equal(xb[:, :T], x) and (xb[:, T:] == 7.0).all() and torch.equal(gb[:, :Tout], g)
    return yb[:, :Tout].clone(), db[:, :T].clone()


def _reference(pair, x, g, lens):
    """float64 (y, d_x) of the restatement and the float32 torch run's relative L2 errors against them."""
    out = {}
    for dt in (torch.float64, torch.float32):
        xv = x.detach().to(dt).clone().requires_grad_(True)
        y = rr.resample(xv, *pair, lengths=lens)
        (gx,) = torch.autograd.grad(y, xv, g.to(dt))
        out[dt] = (y.detach(), gx)
    y64, gx64 = out[torch.float64]
    return y64, gx64, rr.rel_l2(out[torch.float32][0], y64), rr.rel_l2(out[torch.float32][1], gx64)


def _lengths_of(pair):
    o = rr.geometry(*pair)[0]
    return [1, 5, 3 * o, 3 * o + 1, 2125]


def _check_case(pair, x, g, lens, got):
    y, dx = got
    y64, gx64, ef, eb = _reference(pair, x, g, lens)
    rf, rb = rr.rel_l2(y, y64), rr.rel_l2(dx, gx64)
    print("\nFIGURE %s T=%d lens=%s: forward %.3e (float32 torch %.3e), backward %.3e (float32 torch %.3e)"
          % (pair, x.shape[1], lens, rf, ef, rb, eb))
    assert rf <= 10 * ef and rb <= 10 * eb
    if lens is not None:
        for b, n in enumerate(lens):
            assert not y[b, rr.output_length(*pair, n):].any() and not dx[b, n:].any()
    # <R x, g> = <x, R^T g>: both launches read the same float32 coefficients, so the two sides differ by the rounding of the
    # sums alone; with each side within 10 e of its exact value the difference is within 10 max(e) (|y||g| + |x||R^T g|)
    # (g beyond the new lengths meets exact zeros of y, x beyond the lengths exact zeros of d_x)
    lhs, rhs = (y.double() * g.double()).sum().item(), (x.double() * dx.double()).sum().item()
    scale = y64.norm().item() * g.double().norm().item() + x.double().norm().item() * gx64.norm().item()
    assert abs(lhs - rhs) <= 10 * max(ef, eb) * scale


@pytest.mark.parametrize("pair", RATIOS)
def test_emulated_kernels_equal_the_restatement(emu, pair):
    with _emulated(emu):
        for T in _lengths_of(pair):
            x = rr.signal(1, T, 100 + T)
            g = rr.signal(1, rr.output_length(*pair, T), 200 + T)
            _check_case(pair, x, g, None, _run(pair, x, g, None))


@pytest.mark.parametrize("pair", RATIOS)
def test_emulated_ragged_batch_equals_each_utterance_alone(emu, pair):
    lens = [1500, 333, 1]
    x = rr.signal(3, 1500, 7)
    g = rr.signal(3, rr.output_length(*pair, 1500), 8)
    with _emulated(emu):
        y, dx = _run(pair, x, g, lens)
        _check_case(pair, x, g, lens, (y, dx))
        again = _run(pair, x, g, lens)
        assert torch.equal(again[0], y) and torch.equal(again[1], dx)
        for b, n in enumerate(lens):
            m = rr.output_length(*pair, n)
            ya, da = _run(pair, x[b:b + 1, :n].contiguous(), g[b:b + 1, :m].contiguous(), None)
            assert torch.equal(ya[0], y[b, :m]) and torch.equal(da[0], dx[b, :n])
        full = _run(pair, x, g, [1500] * 3)
        none = _run(pair, x, g, None)
        assert torch.equal(full[0], none[0]) and torch.equal(full[1], none[1])


def test_both_table_paths_are_taken(emu):
    with _emulated(emu):
        assert audio.Resample(320, 147).table_paths() == ('lds', 'lds')
        assert audio.Resample(*MEMORY_RATIO).table_paths() == ('memory', 'memory')
        npw, lds = native.resample_plan(147, 320, 27, 2 * 14 + 320)
        assert npw % 256 == 0 and 256 <= npw <= 1024 and lds


def test_module_on_the_stand_in(emu):
    """audio.Resample end to end on host tensors in the emulated mode: ranks, lengths, autograd, the identity case."""
    with _emulated(emu):
        mod = audio.Resample(3, 2)
        x = rr.signal(2, 100, 3).requires_grad_(True)
        y, new_len = mod(x, lengths=[100, 40])
        assert y.shape == (2, 67) and new_len == [67, 27] and mod.output_length(100) == 67
        g = rr.signal(2, 67, 4)
        y.backward(g)
        y64, gx64, ef, eb = _reference((3, 2), x.detach(), g, [100, 40])
        assert rr.rel_l2(y.detach(), y64) <= 10 * ef and rr.rel_l2(x.grad, gx64) <= 10 * eb
        assert mod(x.detach()[0]).shape == (67,) and mod(x.detach()[:, None, :]).shape == (2, 1, 67)
        assert torch.equal(audio.resample(x.detach(), 3, 2), mod(x.detach()))
        same = audio.Resample(22050, 22050)
        assert same(x) is x and same(x, lengths=[100, 40])[1] == [100, 40]
        with pytest.raises(TypeError, match="float32"):
            mod(x.detach().double())
        with pytest.raises(ValueError, match="samples"):
            mod(torch.zeros(2, 2, 5))
        with pytest.raises(ValueError, match="lengths"):
            mod(x.detach(), lengths=[100, 101])
    for bad in ((0, 5), (5, -1)):
        with pytest.raises(ValueError, match="positive"):
            audio.Resample(*bad)


def test_host_tensors_are_refused():
    with pytest.raises(native.NativeError, match="no CPU path"):
        audio.Resample(3, 2)(torch.zeros(1, 10))


def test_refusals(emu):
    tb = _tables((3, 2))
    buf = torch.zeros(1, 64)
    with _emulated(emu):
        with pytest.raises(native.NativeError, match="must not be one of the inputs"):
            native.resample_fwd(buf[:, :30], None, buf[:, 20:40], tb["tab"], tb["first"], 3, 2, tb["width"])
        with pytest.raises(native.NativeError, match="must not be one of the inputs"):
            native.resample_bwd(buf[:, 20:40], None, buf[:, :30], tb["btab"], tb["bfirst"], 3, 2, tb["wpad"], tb["Kd"])
        with pytest.raises(native.NativeError, match=r"ceil\(n T / o\)"):
            native.resample_fwd(torch.zeros(1, 30), None, torch.zeros(1, 21), tb["tab"], tb["first"], 3, 2, tb["width"])
        with pytest.raises(native.NativeError, match="2\\^24 taps"):
            native.resample_plan(1 << 20, 3, 17, 40)
        with pytest.raises(native.NativeError, match="exceeds 4096 samples"):
            native.resample_plan(1, 4000, 100, 8000)
        with pytest.raises(native.NativeError, match="exceeds 4096 samples"):
            audio.Resample(48000, 100).table_paths()
    # rows of 2^31 samples: refused before anything is read (the pointers are never dereferenced)
    p = ctypes.c_void_p(buf.data_ptr())
    big = 1 << 31
    rc = emu.t2amd_resample_fwd_f32(p, big, None, 1, big, p, big, big, p, p, 1, 1, 13, 7, None)
    assert rc != 0 and b"2^31" in emu.t2amd_last_error()
    rc = emu.t2amd_resample_bwd_f32(p, big, None, 1, big, big, p, big, p, p, 1, 1, 13, 7, 20, None)
    assert rc != 0 and b"2^31" in emu.t2amd_last_error()
    rc = emu.t2amd_resample_fwd_f32(p, big - 1, None, 1, big - 1, p, big - 1, big - 1, p, p, 1, 1, 13, 7, None)
    assert rc != 0 and b"2^31" in emu.t2amd_last_error()


# ---- the corpus tool ---------------------------------------------------------------------------------------------------------
def _ref_fn(batch, orig, new, lengths):
    y = rr.resample(torch.from_numpy(batch).double(), orig, new, lengths=lengths)
    return y.numpy(), [rr.output_length(orig, new, n) for n in lengths]


def test_convert(tmp_path):
    from scipy.io.wavfile import read, write
    t = np.arange(3000)
    waves = {"a": (48000, 32767 * np.sign(np.sin(2 * np.pi * 440 * (t + 0.5) / 48000))),     # full scale: rings past it when converted
             "b": (48000, 9000 * np.sin(2 * np.pi * 300 * t[:1234] / 48000)),
             "c": (16000, 12000 * np.sign(np.sin(2 * np.pi * 200 * t[:801] / 16000)))}
    lines = []
    for name, (sr, w) in waves.items():
        write(str(tmp_path / (name + ".wav")), sr, w.astype(np.int16))
        lines.append("%s|text of %s|%s" % (tmp_path / (name + ".wav"), name, name.upper()))
    flist = tmp_path / "list.txt"
    flist.write_text("\n".join(lines) + "\n", encoding="utf-8")
    out = tmp_path / "out"
    calls = []

    def fn(batch, orig, new, lengths):
        calls.append((orig, batch.shape, list(lengths)))
        return _ref_fn(batch, orig, new, lengths)

    written = tool.convert(str(flist), 22050, str(out), batch=2, resample_fn=fn)
    assert calls == [(16000, (1, 801), [801]), (48000, (2, 3000), [3000, 1234])]
    got_lines = (out / "list.txt").read_text(encoding="utf-8").splitlines()
    for (name, (sr, w)), (dst, T), line in zip(waves.items(), written, got_lines):
        rate, pcm = read(dst)
        want_T = rr.output_length(sr, 22050, len(w))
        assert rate == 22050 and pcm.dtype == np.int16 and pcm.shape == (want_T,) and T == want_T
        assert line.split("|") == [str(out / (name + ".wav")), "text of " + name, name.upper()]
        ref = rr.resample(torch.from_numpy(w.astype(np.int16).astype(np.float64))[None], sr, 22050)[0].numpy()
        assert np.array_equal(pcm, np.clip(np.rint(ref), -32768, 32767).astype(np.int16))
    a = read(written[0][0])[1]
    ref_a = rr.resample(torch.from_numpy(waves["a"][1].astype(np.int16).astype(np.float64))[None], 48000, 22050)[0]
    assert ref_a.max() > 32767 and ref_a.min() < -32768 and a.max() == 32767 and a.min() == -32768   # the square wave's ringing clips
    # a file already at the target rate is rewritten unchanged, and no converter is needed for it
    same = tool.convert(str(flist), 48000, str(tmp_path / "same"), batch=4, resample_fn=fn)
    assert np.array_equal(read(same[1][0])[1], waves["b"][1].astype(np.int16)) and read(same[1][0])[0] == 48000
    with pytest.raises(ValueError, match="positive"):
        tool.convert(str(flist), 0, str(out))
