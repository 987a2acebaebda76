"""The multi-resolution STFT loss without a GPU: the margins of the parity inputs that the GPU tests run, the float64 restatement
(tests/stft_loss_ref.py) under gradcheck and at its three defined subgradients, csrc/stft_loss.hip itself run on the host stand-in
against the restatement, and the host plumbing (refusals, launches, kept state, the driver's new keys) in validate-only mode."""
import contextlib
import ctypes
import importlib.util
import os

import pytest
import torch

import golden_util as gu
import stft_loss_ref as sr
from tacotron2_amd import audio, native
from tacotron2_amd import vocos_train as vt


# ---- the condition on the parity inputs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_parity_inputs_keep_their_margins(name):
    """Float32 and float64 agree on the sign of ln m_x - ln m_y in every counted bin, every |ln m_x - ln m_y| is at least 30 x its
    own float32-vs-float64 difference, and no power lies within [eps / 10, 10 eps] of the clamp."""
    B, T, lens = sr.CASES[name]
    x, y = sr.signals(name)
    assert x.shape == (B, T) and y.abs().max() <= 1.0
    eps = sr.PARITY_EPS
    for res in sr.RESOLUTIONS:
        mask = sr.frame_mask(B, T, res, lens)
        d = {}
        for dt in (torch.float32, torch.float64):
            px, mx = sr.power_mag(sr.spectrum(x.to(dt), res), eps)
            py, my = sr.power_mag(sr.spectrum(y.to(dt), res), eps)
            d[dt] = (torch.log(mx) - torch.log(my))[mask].double()
            for p in (px, py):
                p = p[mask]
                assert not ((p >= eps / 10) & (p <= 10 * eps)).any(), (name, res)
        d32, d64 = d[torch.float32], d[torch.float64]
        assert torch.equal(torch.sign(d32), torch.sign(d64)), (name, res)
        ratio = (d64.abs() / (d32 - d64).abs().clamp(min=1e-300)).min().item()
        print("\nFIGURE %s %s: smallest |d| / |d32 - d64| = %.1f, smallest power %.3e" % (name, res, ratio, min(px[mask].min(), py[mask].min())))
        assert ratio >= sr.MARGIN, (name, res, ratio)


# ---- the restatement -----------------------------------------------------------------------------------------------------
TINY = ((16, 4, 12), (8, 3, 8))


def test_restatement_gradcheck():
    g = torch.Generator().manual_seed(3)
    x = (0.1 * torch.randn(2, 21, generator=g, dtype=torch.float64)).requires_grad_(True)
    y = 0.7 * x.detach() + 0.07 * torch.randn(2, 25, generator=g, dtype=torch.float64)[:, :21]
    for lens in (None, [21, 9]):
        assert torch.autograd.gradcheck(lambda v: sr.loss(v, y, TINY, lens, 0.8, 1.3, 1e-12)[0], (x,), eps=1e-7, atol=1e-7)
    val, terms = sr.loss(x, y, TINY, None, 0.8, 1.3, 1e-12)
    assert terms.shape == (2, 2) and abs(val.item() - (0.8 * terms[:, 0] + 1.3 * terms[:, 1]).mean().item()) < 1e-15


def test_restatement_subgradient_definitions():
    g = torch.Generator().manual_seed(5)
    x = 0.1 * torch.randn(1, 40, generator=g, dtype=torch.float64)
    # y = x: A == 0, the spectral-convergence term is the constant 0 and nothing is NaN
    val, terms, grad = sr.loss_and_grad(x, x.clone(), TINY)
    assert val.item() == 0.0 and not terms.any() and torch.isfinite(grad).all() and not grad.any()
    # on spectra: bin (0, 0, 1) below eps, bin (0, 1, 2) of equal magnitudes
    F = 9
    sx = torch.randn(1, 5, 2 * F, generator=g, dtype=torch.float64)
    sy = torch.randn(1, 5, 2 * F, generator=g, dtype=torch.float64)
    sx[0, 0, 1], sx[0, 0, F + 1] = 1e-5, -1e-5                              # p = 2e-10 < eps = 1e-7
    sy[0, 1, 2], sy[0, 1, F + 2] = sx[0, 1, F + 2], sx[0, 1, 2]             # re and im swapped: the same power
    sx.requires_grad_(True)
    mask = torch.ones(1, 5, dtype=torch.bool)
    val, _ = sr.loss_from_spectra([sx], [sy], [mask], 1.0, 1.0, 1e-7)
    val.backward()
    assert torch.isfinite(sx.grad).all()
    assert sx.grad[0, 0, 1] == 0.0 and sx.grad[0, 0, F + 1] == 0.0
    assert sx.grad[0, 1, 2] == 0.0 and sx.grad[0, 1, F + 2] == 0.0          # m_x == m_y: no sc share, sign(0) = 0
    on_eps = torch.zeros(1, 1, 2, dtype=torch.float64)
    on_eps[0, 0, 0] = 0.25
    on_eps.requires_grad_(True)
    sr.loss_from_spectra([on_eps], [torch.ones(1, 1, 2, dtype=torch.float64)], [mask[:, :1]], 1.0, 1.0, 0.0625)[0].backward()
    assert on_eps.grad[0, 0, 0] != 0.0                                      # p == eps: the gradient passes
    with pytest.raises(ValueError, match="all-silent"):
        sr.loss_from_spectra([sx.detach()], [torch.zeros_like(sy)], [mask], 1.0, 1.0, 0.0)
    assert torch.isfinite(sr.loss(x, torch.zeros_like(x), TINY)[0])          # with eps > 0 a silent target has m_y = sqrt(eps)


# ---- csrc/stft_loss.hip on the host stand-in ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loss_emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_stft_loss_emu",
                                                  os.path.join(gu.ROOT, "tests", "hip_emu", "build_stft_loss_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    emu = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("stft_loss_emu"))))
    assert emu.t2amd_emulated() == 1
    for name, at in native._argtypes().items():
        if hasattr(emu, name):
            fn = getattr(emu, name)
            fn.argtypes, fn.restype = at, ctypes.c_int
    emu.t2amd_last_error.restype = ctypes.c_char_p
    return emu


@contextlib.contextmanager
def _emulated(emu):
    saved = (native._lib, native._validate_only)
    native._lib, native._validate_only = emu, True            # CPU pointers allowed, kernels DO run (emulated)
    try:
        yield
    finally:
        native._lib, native._validate_only = saved


def _near(got, want, tol):
    assert got.shape == want.shape
    assert (got.double() - want.double()).abs().max().item() <= tol * max(1e-30, want.abs().max().item())


EMU_CASES = {'A': (sr.signals('A'), None), 'ragged': (tuple(s[:2, :333] for s in sr.signals('C')), (333, 77))}


@pytest.mark.parametrize("name", sorted(EMU_CASES))
def test_emulated_kernels_equal_the_restatement(loss_emu, name):
    """Forward sums, the finish launch's three outputs and d_spec against float64 autograd of the restatement on the very float32
    spectra the kernels read: the differences are the float32 operations of the kernels (magnitudes, logarithms, quotients)."""
    (x, y), lens = EMU_CASES[name]
    B, T = x.shape
    eps, scw, magw, up = 1e-7, 0.8, 1.3, 0.7
    R = len(sr.RESOLUTIONS)
    rows_x = [sr.spec_rows(x, r) for r in sr.RESOLUTIONS]
    rows_y = [sr.spec_rows(y, r) for r in sr.RESOLUTIONS]
    F0 = sr.RESOLUTIONS[0][0] // 2 + 1
    rows_x[0][1, 3], rows_x[0][1, F0 + 3] = 1e-5, -1e-5                             # below eps: no gradient
    rows_y[0][2, 4], rows_y[0][2, F0 + 4] = rows_x[0][2, F0 + 4], rows_x[0][2, 4]   # equal magnitudes: sign 0, no sc share
    cnts = [sr.frame_counts(B, T, r, lens) for r in sr.RESOLUTIONS]
    cnt = torch.tensor(cnts, dtype=torch.int32)
    offs, counts = [0], []
    with _emulated(loss_emu):
        for r, (L, hop, _) in enumerate(sr.RESOLUTIONS):
            offs.append(offs[-1] + native.stft_loss_slots(rows_x[r].shape[0], L // 2 + 1))
            counts.append((L // 2 + 1) * sum(cnts[r]))
        slots = torch.full((3 * offs[-1] + 3,), 7.0, dtype=torch.float64)             # every slot poisoned, one guard slot behind
        again = torch.full((3 * offs[-1] + 3,), -3.0, dtype=torch.float64)            # another poison: an unwritten slot would differ
        for buf in (slots, again):
            for r, (L, hop, _) in enumerate(sr.RESOLUTIONS):
                native.stft_loss_fwd(rows_x[r], rows_y[r], cnt[r], T // hop + 1, L // 2 + 1, eps, buf[3 * offs[r]:3 * offs[r + 1]])
        loss, terms, coef = torch.full((1,), 7.0), torch.full((R, 2), 7.0), torch.full((R, 2), 7.0)
        native.stft_loss_finish(slots[:3 * offs[-1]], offs, counts, scw, magw, loss, terms, coef)
        d_specs = []
        for r, (L, hop, _) in enumerate(sr.RESOLUTIONS):
            d = torch.full((rows_x[r].shape[0], (L + 2 + 31) // 32 * 32), 7.0)
            native.stft_loss_bwd(rows_x[r], rows_y[r], cnt[r], coef[r], torch.tensor([up]), T // hop + 1, L // 2 + 1, eps, d)
            d_specs.append(d)
    assert torch.equal(slots[:3 * offs[-1]], again[:3 * offs[-1]]) and torch.isfinite(slots).all()
    assert (slots[3 * offs[-1]:] == 7.0).all() and (again[3 * offs[-1]:] == -3.0).all()
    # the restatement on the same spectra
    sx = [rx.double().view(B, -1, rx.shape[1]).requires_grad_(True) for rx in rows_x]
    sy = [ry.double().view(B, -1, ry.shape[1]) for ry in rows_y]
    masks = [sr.frame_mask(B, T, r, lens) for r in sr.RESOLUTIONS]
    want, want_terms = sr.loss_from_spectra(sx, sy, masks, scw, magw, eps)
    (want * up).backward()
    for r in range(R):
        A, Bn, Lm = (v.item() for v in sr.sums(sx[r].detach(), sy[r], masks[r], eps))
        got = slots[3 * offs[r]:3 * offs[r + 1]].view(-1, 3).sum(0)
        assert abs(got[0].item() - A) <= 1e-6 * A and abs(got[1].item() - Bn) <= 1e-6 * Bn and abs(got[2].item() - Lm) <= 1e-5 * Lm
        assert abs(coef[r, 0].item() - scw / (R * (A * Bn) ** 0.5)) <= 2e-6 * coef[r, 0].item()
        assert abs(coef[r, 1].item() - magw / (R * counts[r])) <= 2e-7 * coef[r, 1].item()
        F = sr.RESOLUTIONS[r][0] // 2 + 1
        d = d_specs[r]
        _near(d[:, :2 * F], sx[r].grad.view(-1, 2 * F), 2e-5)
        assert not d[:, 2 * F:].any()                                                 # the padding columns
        outside = ~masks[r].reshape(-1)
        assert not d[outside].any() and (lens is None or outside.any())               # the masked frames
    _near(terms, want_terms, 1e-5)
    assert abs(loss.item() - want.item()) <= 1e-5 * want.item()
    assert d_specs[0][1, 3] == 0.0 and d_specs[0][1, F0 + 3] == 0.0
    g_eq = sx[0].grad.view(-1, 2 * F0)[2, 4].item()
    assert g_eq == 0.0 and d_specs[0][2, 4] == 0.0 and d_specs[0][2, F0 + 4] == 0.0


@pytest.mark.parametrize("B,n,F,lens,nslots", [(2, 1500, 17, (1500, 611), 4), (2, 130, 257, (130, 47), 5)])
def test_emulated_kernels_over_many_slots(loss_emu, B, n, F, lens, nslots):
    """Several workgroups per resolution: random spectra (the row kernels do not care where a spectrum came from), ragged frame
    counts, a tail workgroup with fewer rows than the others, two resolutions in one finish launch (the second a short one, so the
    offsets matter).  Every slot is poisoned with a value of its own, differently in the two runs.  (More than 256 slots through
    the forward cost minutes on the stand-in: the finish launch's strided loop has the test below, the composition the GPU
    suite's many-slot case.)"""
    g = torch.Generator().manual_seed(100 + F)
    eps, scw, magw, up = 1e-7, 0.8, 1.3, 0.7
    rows = B * n
    assert rows % ((16384 + F - 1) // F) != 0                  # the last workgroup is a partial one
    sx, sy = 0.1 * torch.randn(rows, 2 * F, generator=g), 0.1 * torch.randn(rows, 2 * F, generator=g)
    sx2, sy2 = 0.1 * torch.randn(7, 10, generator=g), 0.1 * torch.randn(7, 10, generator=g)       # a second resolution: 1 x 7 x 5
    cnt = torch.tensor(lens, dtype=torch.int32)
    cnt2 = torch.tensor([6], dtype=torch.int32)
    with _emulated(loss_emu):
        ns = native.stft_loss_slots(rows, F)
        assert ns == nslots and native.stft_loss_slots(7, 5) == 1
        offs, counts = [0, ns, ns + 1], [F * sum(lens), 5 * 6]
        bufs = [torch.arange(3 * ns + 6, dtype=torch.float64) * 1e3 + 7.0, -torch.arange(3 * ns + 6, dtype=torch.float64) - 3.0]
        poison = [b.clone() for b in bufs]
        for buf in bufs:
            native.stft_loss_fwd(sx, sy, cnt, n, F, eps, buf[:3 * ns])
            native.stft_loss_fwd(sx2, sy2, cnt2, 7, 5, eps, buf[3 * ns:3 * ns + 3])
        slots = bufs[0]
        loss, terms, coef = torch.full((1,), 7.0), torch.full((2, 2), 7.0), torch.full((2, 2), 7.0)
        native.stft_loss_finish(slots[:3 * ns + 3], offs, counts, scw, magw, loss, terms, coef)
        Kp = (2 * F + 31) // 32 * 32
        d = torch.full((rows, Kp), 7.0)
        native.stft_loss_bwd(sx, sy, cnt, coef[0], torch.tensor([up]), n, F, eps, d)
    owned = 3 * ns + 3
    assert torch.equal(bufs[0][:owned], bufs[1][:owned])
    assert torch.equal(bufs[0][owned:], poison[0][owned:]) and torch.equal(bufs[1][owned:], poison[1][owned:])
    # the restatement: per-slot sums against the rows each workgroup owns, then the whole
    rpb = -(-16384 // F)
    mask = torch.arange(n)[None, :] < cnt[:, None]
    x64 = sx.double().view(B, n, 2 * F).requires_grad_(True)
    y64 = sy.double().view(B, n, 2 * F)
    x2, y2, m2 = sx2.double().view(1, 7, 10).requires_grad_(True), sy2.double().view(1, 7, 10), torch.arange(7)[None, :] < 6
    for s in (0, 1, ns - 1):
        r0, r1 = s * rpb, min(rows, (s + 1) * rpb)
        want = sr.sums(sx.double()[r0:r1], sy.double()[r0:r1], mask.reshape(-1)[r0:r1], eps)
        for k in range(3):
            assert abs(slots[3 * s + k].item() - want[k].item()) <= 1e-6 * max(want[k].item(), 1e-30), (s, k)
    want, want_terms = sr.loss_from_spectra([x64, x2], [y64, y2], [mask, m2], scw, magw, eps)
    (want * up).backward()
    A, Bn, Lm = (v.item() for v in sr.sums(x64.detach(), y64, mask, eps))
    got = slots[:3 * ns].view(-1, 3).sum(0)
    assert abs(got[0].item() - A) <= 1e-6 * A and abs(got[1].item() - Bn) <= 1e-6 * Bn and abs(got[2].item() - Lm) <= 1e-5 * Lm
    _near(terms, want_terms, 1e-5)
    assert abs(loss.item() - want.item()) <= 1e-5 * want.item()
    assert abs(coef[0, 0].item() - scw / (2 * (A * Bn) ** 0.5)) <= 2e-6 * coef[0, 0].item()
    assert abs(coef[0, 1].item() - magw / (2 * counts[0])) <= 2e-7 * coef[0, 1].item()
    assert abs(coef[1, 1].item() - magw / (2 * counts[1])) <= 2e-7 * coef[1, 1].item()
    _near(d[:, :2 * F], x64.grad.view(rows, 2 * F), 2e-5)
    assert not d[:, 2 * F:].any() and not d[~mask.reshape(-1)].any()


@pytest.mark.parametrize("ns", [(5, 257, 3), (700, 1, 256)])
def test_emulated_finish_over_many_slots(loss_emu, ns):
    """stft_loss_finish alone on slots of known values: up to 700 slots per resolution (its stride-256 loop runs three times, the
    last partly; all four waves carry sums), three resolutions at their offsets, against float64 sums of the same slots."""
    g = torch.Generator().manual_seed(9)
    offs = [0]
    for k in ns:
        offs.append(offs[-1] + k)
    slots = torch.rand(3 * offs[-1] + 3, generator=g, dtype=torch.float64) + 0.5
    slots[3 * offs[-1]:] = float('nan')                                               # a guard slot that must not be read
    counts = [1000.0 * k for k in ns]
    with _emulated(loss_emu):
        loss, terms, coef = torch.full((1,), 7.0), torch.full((3, 2), 7.0), torch.full((3, 2), 7.0)
        native.stft_loss_finish(slots[:3 * offs[-1]], offs, counts, 0.8, 1.3, loss, terms, coef)
    total = 0.0
    for r in range(3):
        A, Bn, Lm = (v.item() for v in slots[3 * offs[r]:3 * offs[r + 1]].view(-1, 3).sum(0))
        sc, lm = (A / Bn) ** 0.5, Lm / counts[r]
        assert abs(terms[r, 0].item() - sc) <= 2e-7 * sc and abs(terms[r, 1].item() - lm) <= 2e-7 * lm
        assert abs(coef[r, 0].item() - 0.8 / (3 * (A * Bn) ** 0.5)) <= 2e-7 * coef[r, 0].item()
        assert abs(coef[r, 1].item() - 1.3 / (3 * counts[r])) <= 2e-7 * coef[r, 1].item()
        total += 0.8 * sc + 1.3 * lm
    assert abs(loss.item() - total / 3) <= 2e-7 * total / 3


def test_emulated_zero_difference_and_sum(loss_emu):
    """y = x: A == 0 gives sc = 0, coefficient 0 and a d_spec of exact zeros; the summing launch adds in the order r = 0 .. R - 1."""
    x, _ = sr.signals('A')
    res = sr.RESOLUTIONS[1]
    L, hop, F = res[0], res[1], res[0] // 2 + 1
    rows = sr.spec_rows(x, res)
    n = rows.shape[0]
    cnt = torch.tensor([n], dtype=torch.int32)
    with _emulated(loss_emu):
        ns = native.stft_loss_slots(n, F)
        slots = torch.full((3 * ns,), 7.0, dtype=torch.float64)
        native.stft_loss_fwd(rows, rows.clone(), cnt, n, F, 1e-7, slots)
        loss, terms, coef = torch.empty(1), torch.empty(1, 2), torch.empty(1, 2)
        native.stft_loss_finish(slots, [0, ns], [F * n], 1.0, 1.0, loss, terms, coef)
        d = torch.full((n, (2 * F + 31) // 32 * 32), 7.0)
        native.stft_loss_bwd(rows, rows.clone(), cnt, coef[0], torch.ones(1), n, F, 1e-7, d)
        parts = torch.randn(3, 2, 37, generator=torch.Generator().manual_seed(8))
        out = torch.full((2, 37), 7.0)
        native.stft_loss_sum(parts, out)
    assert loss.item() == 0.0 and not terms.any() and coef[0, 0] == 0.0 and coef[0, 1] > 0.0 and not d.any()
    assert torch.equal(out, (parts[0] + parts[1]) + parts[2])


# ---- host plumbing ---------------------------------------------------------------------------------------------------------
def _err(fn, *a, match):
    with pytest.raises(native.NativeError, match=match):
        fn(*a)


def test_entries_reject_bad_arguments(native_lib):
    native.set_validate_only(True)
    try:
        z = torch.zeros
        B, n, F = 2, 5, 17
        R, Kp = B * n, 64
        sx, sy, cnt = z(R, 2 * F), z(R, 2 * F), torch.full((B,), n, dtype=torch.int32)
        ns = native.stft_loss_slots(R, F)
        assert ns == 1 and native.stft_loss_slots(2000, 17) == 3 and native.stft_loss_slots(5, 20000) == 5
        slots = z(3 * ns, dtype=torch.float64)
        native.stft_loss_fwd(sx, sy, cnt, n, F, 1e-7, slots)
        _err(native.stft_loss_fwd, sx, sy, cnt, n, F, 0.0, slots, match="eps")
        _err(native.stft_loss_fwd, sx, sy, cnt, n, F, 1e-7, z(2, dtype=torch.float64), match="slot buffer is shorter")
        _err(native.stft_loss_fwd, sx, z(R + 1, 2 * F), cnt, n, F, 1e-7, slots, match="shape mismatch")
        _err(native.stft_loss_fwd, sx, sy, cnt, n, F + 1, 1e-7, slots, match="shape mismatch")
        _err(native.stft_loss_fwd, sx, sy, cnt.long(), n, F, 1e-7, slots, match="int32")
        _err(native.stft_loss_fwd, sx, sy, None, n, F, 1e-7, slots, match="int32")
        _err(native.stft_loss_fwd, sx, sy, cnt, n, F, 1e-7, z(3 * ns), match="float64")
        loss, terms, coef = z(1), z(3, 2), z(3, 2)
        s9 = z(9, dtype=torch.float64)
        native.stft_loss_finish(s9, [0, 1, 2, 3], [10, 10, 10], 1.0, 1.0, loss, terms, coef)
        _err(native.stft_loss_finish, s9, [0, 1, 2, 4], [10, 10, 10], 1.0, 1.0, loss, terms, coef, match="shorter")
        _err(native.stft_loss_finish, s9, [0, 1, 1, 3], [10, 10, 10], 1.0, 1.0, loss, terms, coef, match="ascend")
        _err(native.stft_loss_finish, s9, [0, 1, 2, 3], [10, 0, 10], 1.0, 1.0, loss, terms, coef, match="count")
        _err(native.stft_loss_finish, s9, [0, 1, 2], [10, 10, 10], 1.0, 1.0, loss, terms, coef, match="offsets")
        _err(native.stft_loss_finish, s9, [0, 1, 2, 3], [10, 10, 10], 1.0, 1.0, loss, terms, terms, match="distinct")
        _err(native.stft_loss_finish, z(30, dtype=torch.float64), list(range(10)), [1] * 9, 1.0, 1.0, loss, z(9, 2), z(9, 2),
             match="1 to 8")
        d = z(R, Kp)
        native.stft_loss_bwd(sx, sy, cnt, z(2), z(1), n, F, 1e-7, d)
        _err(native.stft_loss_bwd, sx, sy, cnt, z(3), z(1), n, F, 1e-7, d, match="coef of 3")
        _err(native.stft_loss_bwd, sx, sy, cnt, z(2), z(2), n, F, 1e-7, d, match="g of 2")
        _err(native.stft_loss_bwd, sx, sy, cnt, z(2), z(1), n, F, 1e-7, z(R, 2 * F - 1), match="shape mismatch")
        _err(native.stft_loss_bwd, sx, sy, cnt, z(2), z(1), n, F, 1e-7, sx, match="must not be one of the inputs")
        _err(native.stft_loss_bwd, sx, sy, cnt, z(2), z(1), n, F, -1.0, d, match="eps")
        parts = z(3, 2, 9)
        native.stft_loss_sum(parts, z(2, 9))
        _err(native.stft_loss_sum, parts, z(2, 8), match="beside out")
        _err(native.stft_loss_sum, parts, parts[1], match="must not lie in parts")
        _err(native.stft_loss_sum, z(9, 2, 9), z(2, 9), match="1 to 8")
    finally:
        native.set_validate_only(False)


def test_module_validate_only(native_lib, monkeypatch):
    """Refusals before any launch, the launches of one forward and backward, the kept state and the second-backward message."""
    native.set_validate_only(True)
    calls = []
    names = ('reflect_pad', 'gemm', 'stft_magnitude', 'stft_loss_fwd', 'stft_loss_finish', 'stft_loss_bwd', 'stft_frames_fold',
             'stft_loss_sum')
    for fn in names:
        real = getattr(native, fn)
        monkeypatch.setattr(native, fn, lambda *a, _f=fn, _r=real, **k: (calls.append((_f, k.get('fast'))), _r(*a, **k))[1])
    try:
        ml = audio.MultiResolutionSTFTLoss()
        assert ml.resolutions == ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240)) and ml.eps == 1e-7
        assert (ml.sc_weight, ml.mag_weight) == (1.0, 1.0) and ml.last_terms is None
        B, T = 2, 2125
        for prec, fast in (('fp32', 0), ('bf16x3', 1)):
            a = torch.zeros(B, 1, T, requires_grad=True)
            del calls[:]
            loss = ml(a, torch.zeros(B, T + 9), lengths=torch.tensor([T, 700]), precision=prec)
            assert loss.dim() == 0 and loss.requires_grad and loss.dtype == torch.float32
            assert [c for c, _ in calls] == ['reflect_pad', 'reflect_pad', 'gemm'] * 3 + ['stft_loss_fwd'] * 3 + ['stft_loss_finish']
            specs, cnt, coef = loss.grad_fn.kept
            assert sum(s.numel() for s in specs) + cnt.numel() + coef.numel() == ml.kept_state_floats(B, T)
            assert cnt.tolist() == [[18, 6], [9, 3], [43, 15]] and tuple(ml.last_terms.shape) == (3, 2)
            assert not ml.last_terms.requires_grad
            del calls[:]
            loss.backward()
            assert calls == [('stft_loss_bwd', None), ('gemm', fast), ('stft_frames_fold', None)] * 3 + [('stft_loss_sum', None)]
            assert a.grad.shape == a.shape and a.grad.dtype == torch.float32
            with pytest.raises(RuntimeError, match="MultiResolutionSTFTLoss: backward was already run"):
                loss.backward()
        del calls[:]
        for bad, match in (((torch.zeros(2, 2, T), torch.zeros(2, T)), r"\(B, T\) or \(B, 1, T\)"),
                           ((torch.zeros(2, T), torch.zeros(3, T)), r"\(2, >= 2125\) target"),
                           ((torch.zeros(2, T), torch.zeros(2, T - 1)), r"\(2, >= 2125\) target"),
                           ((torch.zeros(2, 1024), torch.zeros(2, 1024)), r"1024 samples is too short to reflect-pad by 1024")):
            with pytest.raises(ValueError, match=match):
                ml(*bad)
        for lens, match in (([T], "1 lengths for a batch of 2"), ([0, T], r"\[1, 2125\], got \[0, 2125\]"),
                            ([T + 1, T], r"\[1, 2125\], got \[2126, 2125\]")):
            with pytest.raises(ValueError, match=match):
                ml(torch.zeros(2, T), torch.zeros(2, T), lengths=lens)
        with pytest.raises(ValueError, match="precision must be one of .* got 'bf16'"):
            ml(torch.zeros(2, T), torch.zeros(2, T), precision='bf16')
        assert calls == []                                                   # every refusal came before any launch
        for res, match in ((((64, 16, 65),), r"\(64, 16, 65\)"), (((64, 65, 64),), r"\(64, 65, 64\)"), (((64, 16),), r"\(64, 16\)"),
                           ((), "got 0"), (((64, 16, 48),) * 9, "got 9"), (5, "triples")):
            with pytest.raises(ValueError, match=match):
                audio.MultiResolutionSTFTLoss(res)
        with pytest.raises(ValueError, match="eps"):
            audio.MultiResolutionSTFTLoss(eps=0.0)
        one = audio.MultiResolutionSTFTLoss(((64, 16, 48),))
        x = torch.zeros(1, 65, requires_grad=True)
        del calls[:]
        one(x, torch.zeros(1, 65)).backward()
        assert 'stft_loss_sum' not in [c for c, _ in calls] and x.grad.shape == (1, 65)
    finally:
        native.set_validate_only(False)
    if not torch.cuda.is_available():
        with pytest.raises(native.NativeError, match="move the module to the MI355X first"):
            audio.MultiResolutionSTFTLoss(sr.RESOLUTIONS)(torch.zeros(1, 100), torch.zeros(1, 100))


def test_driver_keys():
    cfg = vt.load_config()
    assert cfg == vt.DEFAULTS and cfg['train_config']['stft_loss_weight'] == 0.0 and cfg['train_config']['stft_resolutions'] is None
    assert vt.check_config(cfg) == (64, 64)
    cfg = vt.load_config(None, ["stft_loss_weight=1.5", "stft_resolutions=[[64,16,48],[32,10,24]]"])
    assert cfg['train_config']['stft_loss_weight'] == 1.5 and cfg['train_config']['stft_resolutions'] == [[64, 16, 48], [32, 10, 24]]
    assert vt.check_config(cfg) == (64, 64)
    assert vt.check_config(vt.load_config(None, ["stft_loss_weight=1"])) == (64, 64)         # the default resolutions fit 16384
    for bad, match in ((["stft_loss_weight=-0.5"], "stft_loss_weight must be a number >= 0, got -0.5"),
                       (["stft_loss_weight=much"], "stft_loss_weight must be a number"),
                       (["stft_loss_weight=1", "segment_length=1024"], "filter_length 2048 reflect-pads by 1024"),
                       (["stft_loss_weight=1", "segment_length=1280", "padding=center", "stft_resolutions=[[2048,240,1200]]"],
                        "the generated audio has 1024 samples"),
                       (["stft_loss_weight=1", "stft_resolutions=[[64,16,65]]"], r"resolution \(64, 16, 65\)")):
        with pytest.raises(ValueError, match=match):
            vt.check_config(vt.load_config(None, bad))
    # with the weight 0 the resolutions are not even looked at
    assert vt.check_config(vt.load_config(None, ["segment_length=1024", "stft_resolutions=[[64,16,65]]"])) == (4, 4)


def test_driver_run_validate_only(native_lib, tmp_path, capsys, monkeypatch):
    """A whole run with the second loss in validate-only mode: every host check of the composed step; without the weight the
    module is never constructed."""
    built = []
    real = audio.MultiResolutionSTFTLoss.__init__
    monkeypatch.setattr(audio.MultiResolutionSTFTLoss, "__init__", lambda self, *a, **k: (built.append(a), real(self, *a, **k))[1])
    tiny = ["vocos_config.dim=32", "intermediate_dim=64", "num_layers=1", "training_files=synthetic:5", "batch_size=2",
            "segment_length=2048", "epochs=1", "iters_per_checkpoint=1", "learning_rate=0.001"]
    native.set_validate_only(True)
    try:
        for extra, n_built in (([], 0), (["stft_loss_weight=1.0", "stft_resolutions=[[64,16,48],[128,40,100],[32,10,24]]"], 1),
                               (["stft_loss_weight=0.5", "padding=center"], 2)):
            out = str(tmp_path / ("out%d" % len(extra)) / str(n_built))
            it, last = vt.main(["--set", "output_directory=" + out] + [a for s in tiny + extra for a in ("--set", s)])
            assert it == 1 and isinstance(last, float) and len(built) == n_built
            ckpt = torch.load(os.path.join(out, 'vocos_1'), map_location='cpu', weights_only=False)
            assert set(ckpt) == {'state_dict', 'iteration', 'optimizer', 'learning_rate', 'vocos_config'}
        lines = [l for l in capsys.readouterr().out.splitlines() if l[:1].isdigit()]
        assert [l.split(':')[0] for l in lines] == ['0', '1'] * 3
    finally:
        native.set_validate_only(False)
