"""The products of the shared MFMA tile loop (csrc/rowmma.h) alone on the MI355X, every client at every precision: vc_linear
(csrc/vocos.hip), hg_conv and hg_upsample (csrc/hifigan.hip), wg_gated, wg_res_skip and wg_dgrad (csrc/waveglow_layer.hip)
against the float64 restatements of tests/rowmma_ref.py, which multiply the operands ROUNDED THE WAY THE KERNEL ROUNDS THEM
(tests/test_rowmma_ref_cpu.py proves them against torch's float64 operators, and that a single wrong tap, term, K-step, column
or row misses the limit used here by more than 100 x).

One rule for every comparison: the figure is the relative L2 of a buffer's computed elements against the float64 restatement of
the same precision, and the limit is 10 x e32, e32 being the larger error of the two float32 runs of the same arithmetic
(torch's matmul, and a plain ascending-k accumulation) through the same epilogue in float32, computed here on the GPU.  10 x is
the project's rule for two f32 sums in different orders; nothing in the limit comes from the code under test.

Every output lies in a buffer that is wider and longer than the kernel's view and filled with 7.0; ldx, ldout, ldres, ldcnd,
ldacts, ldh, ldskip, ldgate and ldhout exceed their widths by 4, 8, ... 36 floats (PAD).  What the restatement does not mark as
computed must come back bit for bit: 7.0 outside the view, zero on halo rows, the old value on rows the kernel skips.  The
operands' pad columns and spare rows hold NaN.

Worst figure / e32 per client and precision, measured on the MI355X (profiles/rowmma_alone_pytest_gpu.txt has the run with every
figure; e32 lies between 1.8e-8 and 7.6e-7).  No precision needed more than the 10 x rule: the MFMA's own accumulation is no
further from float64 than a float32 sum over ascending k.

                   0 (exact f32)   1 (split-bf16 x 3)   2 (bf16)
    vc_linear      1.38            0.71                 1.13
    hg_conv        1.00            0.73                 0.98
    hg_upsample    1.00            0.43                 0.89
    wg_gated       1.02            0.49                 0.95
    wg_res_skip    1.00            0.53                 0.95
    wg_dgrad       1.00            0.39                 0.76"""
import pytest
import torch
import torch.nn.functional as F

import rowmma_ref as rr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PRECS = (0, 1, 2)
FACTOR = {0: 10.0, 1: 10.0, 2: 10.0}                   # limit = FACTOR x e32
PAD = dict(x=4, out=8, res=12, cnd=16, acts=20, h=24, skip=28, gate=32, hout=36)
FILL = 7.0
SPARE = 5                                              # rows of every buffer beyond the view
WORST = {}                                             # (client, precision) -> worst figure / e32


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    yield
    print("\nworst figure / e32 per client and precision (limit %s)" % (FACTOR,))
    for client in sorted({c for c, _ in WORST}):
        print("    %-12s %s" % (client, "   ".join("%d: %5.2f" % (p, WORST[(client, p)]) for p in PRECS if (client, p) in WORST)))


@pytest.fixture(scope="module")
def nv(native_lib):
    from tacotron2_amd import native
    assert torch.cuda.is_available(), "GPU tests need a device"
    return native


def _dev(c):
    return {k: v.to(DEV) if torch.is_tensor(v) else v for k, v in c.items()}


def _operand(t, pad):
    """t as a view of a wider, longer buffer whose other elements are NaN."""
    B = torch.full((t.shape[0] + SPARE, t.shape[1] + pad), float('nan'), device=DEV)
    B[:t.shape[0], :t.shape[1]] = t
    return B[:t.shape[0], :t.shape[1]]


class Out:
    """A [rows][cols] view (v) of a wider, longer buffer of 7.0."""

    def __init__(self, rows, cols, pad, init=None):
        self.B = torch.full((rows + SPARE, cols + pad), FILL, device=DEV)
        self.v = self.B[:rows, :cols]
        if init is not None:
            self.v.copy_(init)

    def untouched_outside(self):
        c = self.B.clone()
        c[:self.v.shape[0], :self.v.shape[1]] = FILL
        return bool((c == FILL).all())


def _judge(client, tag, prec, got, fn, bad, parts=None):
    """got {name: Out or tensor} against fn(mm) -> {name: (expected, computed)}; failures go to `bad`, every figure is printed."""
    want = fn(rr.product)
    w32 = [fn(mm) for mm in rr.F32_PRODUCTS]
    for name, (exp, mask) in want.items():
        g = got[name]
        if isinstance(g, Out):
            if not g.untouched_outside():
                bad.append((tag, name, "written outside the view"))
            g = g.v
        assert g.dtype == torch.float32 and g.shape == exp.shape and exp.dtype == torch.float64
        if not torch.equal(g[~mask], exp[~mask].float()):
            bad.append((tag, name, "an element the kernel must leave alone or write as zero differs"))
        if not mask.any():
            continue
        for label, idx in [("", slice(None))] + list((parts or {}).items()):
            m = mask[idx]
            fig = rr.rel(g[idx][m], exp[idx][m])
            e32 = max(rr.rel(w[name][0][idx][m], exp[idx][m]) for w in w32)
            assert e32 > 0, (tag, name, label)
            print("%s precision %d %s %s%s: relative L2 %.3g, e32 %.3g, ratio %.2f" % (client, prec, tag, name, label, fig, e32,
                                                                                         fig / e32))
            WORST[(client, prec)] = max(WORST.get((client, prec), 0.0), fig / e32)
            if not fig < FACTOR[prec] * e32:
                bad.append((tag, name + label, fig, e32))


# ---- Vocos: vc_linear -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", rr.VC_K)
@pytest.mark.parametrize("prec", PRECS)
def test_vc_linear_alone(nv, prec, K):
    bad = []
    for N in rr.VC_N:
        for lens in rr.VC_LENS:
            c = _dev(rr.make_vc(K, N, lens))
            P, W, b, gamma, rowb0 = c['P'], c['W'], c['bias'], c['gamma'], c['rowb0']
            X, res = _operand(c['X'], PAD['x']), _operand(c['res'], PAD['res'])
            tag = "K=%d N=%d P=%d" % (K, N, P)
            for epi in (None, 'gelu', 'residual'):
                out = Out(P, N, PAD['out'])
                nv.vc_linear(X, W, b, epi, gamma if epi else None, res if epi == 'residual' else None, out.v, rowb0, prec)
                _judge("vc_linear", "%s epi=%s" % (tag, epi), prec, {'out': out},
                       lambda mm: rr.vc_linear_ref(X, W, b, epi, gamma, res, rowb0, prec, mm), bad)
                again = Out(P, N, PAD['out'])
                nv.vc_linear(X, W, b, epi, gamma if epi else None, res if epi == 'residual' else None, again.v, rowb0, prec)
                if not torch.equal(again.B, out.B):
                    bad.append((tag, epi, "two calls differ"))
                if epi == 'residual':                               # in place, as the layer loop runs it
                    y = Out(P, N, PAD['out'], init=c['res'])
                    nv.vc_linear(X, W, b, epi, gamma, y.v, y.v, rowb0, prec)
                    if not torch.equal(y.B, out.B):
                        bad.append((tag, epi, "res aliased to out differs from res beside out"))
    assert not bad, bad


# ---- HiFi-GAN: hg_conv, hg_upsample -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d,Cin,N", rr.HG_CONV)
@pytest.mark.parametrize("prec", PRECS)
def test_hg_conv_alone(nv, prec, k, d, Cin, N):
    from tacotron2_amd.hifigan import pack_conv
    c = _dev(rr.make_hg_conv(k, d, Cin, N))
    P, S, w, b, rowb0 = c['P'], c['S'], c['w'], c['bias'], c['rowb0']
    X, R = _operand(c['X'], PAD['x']), _operand(c['res'], PAD['res'])
    wp, bp = pack_conv(w, b, Cin, N)
    tag, bad = "k=%d d=%d Cin=%d N=%d" % (k, d, Cin, N), []

    def ref(res, scale, out0, accumulate):
        return lambda mm: rr.hg_conv_ref(X, w, b, d, rr.SLOPE, res, scale, out0, accumulate, rowb0, S, prec, mm)

    out, acc = Out(P, N, PAD['out']), Out(P, N, PAD['out'])
    nv.hg_conv(X, wp, bp, k, d, rr.SLOPE, None, out.v, 1.0, False, rowb0, S, prec)
    _judge("hg_conv", tag + " store", prec, {'out': out}, ref(None, 1.0, None, False), bad)
    nv.hg_conv(X, wp, bp, k, d, rr.SLOPE, R, acc.v, 1.0, False, rowb0, S, prec)
    _judge("hg_conv", tag + " residual", prec, {'out': acc}, ref(R, 1.0, None, False), bad)
    before = acc.v.clone()
    nv.hg_conv(X, wp, bp, k, d, rr.SLOPE, R, acc.v, 0.5, True, rowb0, S, prec)
    _judge("hg_conv", tag + " accumulate", prec, {'out': acc}, ref(R, 0.5, before, True), bad)
    again = Out(P, N, PAD['out'])
    nv.hg_conv(X, wp, bp, k, d, rr.SLOPE, None, again.v, 1.0, False, rowb0, S, prec)
    assert torch.equal(again.B, out.B), "two calls must give the same bits"
    assert not bad, bad


@pytest.mark.parametrize("ci,co,ku,u", rr.HG_UP)
@pytest.mark.parametrize("prec", PRECS)
def test_hg_upsample_alone(nv, prec, ci, co, ku, u):
    from tacotron2_amd.hifigan import pack_up
    c = _dev(rr.make_hg_up(ci, co, ku, u))
    P, S, w, b, rowb0 = c['P'], c['S'], c['w'], c['bias'], c['rowb0']
    X = _operand(c['X'], PAD['x'])
    wp, bp = pack_up(w, b, u, ci, co)
    bad = []
    out, again = Out(P * u, co, PAD['out']), Out(P * u, co, PAD['out'])
    nv.hg_upsample(X, wp, bp, ku, u, rr.SLOPE, out.v, rowb0, S, prec)
    nv.hg_upsample(X, wp, bp, ku, u, rr.SLOPE, again.v, rowb0, S, prec)
    _judge("hg_upsample", "ci=%d co=%d ku=%d u=%d" % (ci, co, ku, u), prec, {'out': out},
           lambda mm: rr.hg_upsample_ref(X, w, b, u, rr.SLOPE, rowb0, S, prec, mm), bad,
           parts={" phase %d" % ph: slice(ph, None, u) for ph in range(u)})
    assert torch.equal(again.B, out.B), "two calls must give the same bits"
    assert not bad, bad


# ---- WaveGlow: wg_gated, wg_res_skip, wg_dgrad -----------------------------------------------------------------------------
@pytest.mark.parametrize("C,dil,M", rr.WG_GATED)
@pytest.mark.parametrize("prec", PRECS)
def test_wg_gated_alone(nv, prec, C, dil, M):
    c = _dev(rr.make_wg_gated(C, dil, M))
    w, b = c['w'], c['bias']
    perm = rr.gate_perm(C).to(DEV)
    wp, bp = w.permute(0, 2, 1).reshape(2 * C, 3 * C)[perm].contiguous(), b[perm].contiguous()
    img, cnd = _operand(c['img'], PAD['x']), _operand(c['cnd'], PAD['cnd'])
    X = img[dil:dil + M]                                          # the image goes on, zero, for dil rows on both sides
    bad = []
    plain, acts, gate = Out(M, C, PAD['acts']), Out(M, C, PAD['acts']), Out(M, 2 * C, PAD['gate'])
    nv.wg_gated(X, wp, bp, dil, cnd, plain.v, prec)
    nv.wg_gated(X, wp, bp, dil, cnd, acts.v, prec, gate=gate.v)
    _judge("wg_gated", "C=%d dil=%d M=%d" % (C, dil, M), prec, {'acts': acts, 'gate': gate},
           lambda mm: rr.wg_gated_ref(img, dil, M, w, b, dil, cnd, prec, mm), bad)
    assert torch.equal(plain.B, acts.B), "acts must have the same bits with and without gate"
    assert torch.equal(gate.v[:, :C] * gate.v[:, C:], acts.v), "acts must be the product of the two gate values kept"
    assert not bad, bad


@pytest.mark.parametrize("C,N,nres", rr.WG_RES_SKIP)
@pytest.mark.parametrize("prec", PRECS)
def test_wg_res_skip_alone(nv, prec, C, N, nres):
    c = _dev(rr.make_wg_res_skip(C, N, nres))
    M, W, b, rowb, h0 = rr.WG_M, c['W'], c['bias'], c['rowb'], c['h0']
    acts = _operand(c['acts'], PAD['x'])
    real = rowb >= 0
    tag, bad = "C=%d N=%d nres=%d" % (C, N, nres), []

    def ref(h_now, skip_now, store, h_out0=None):
        return lambda mm: rr.wg_res_skip_ref(acts, W, b, h_now, skip_now, store, rowb, prec, mm, h_out0=h_out0)

    h = Out(M, nres, PAD['h'], init=h0) if nres else None
    skip = Out(M, N - nres, PAD['skip'])
    nv.wg_res_skip(acts, W, b, h.v if nres else None, skip.v, True, rowb, prec)
    _judge("wg_res_skip", tag + " store", prec, {'h': h, 'skip': skip}, ref(h0, None, True), bad)
    h1, skip1 = (h.v.clone() if nres else None), skip.v.clone()
    nv.wg_res_skip(acts, W, b, h.v if nres else None, skip.v, False, rowb, prec)
    _judge("wg_res_skip", tag + " add", prec, {'h': h, 'skip': skip}, ref(h1, skip1, False), bad)
    if nres:                                                      # the training forward: h_out beside an unchanged h
        hb, hout, skipb = Out(M, nres, PAD['h'], init=h0), Out(M, nres, PAD['hout']), Out(M, N - nres, PAD['skip'])
        nv.wg_res_skip(acts, W, b, hb.v, skipb.v, True, rowb, prec, h_out=hout.v)
        _judge("wg_res_skip", tag + " h_out", prec, {'h': hb, 'h_out': hout, 'skip': skipb},
               ref(h0, None, True, h_out0=torch.full_like(h0, FILL)), bad)
        assert torch.equal(hb.v, h0), "h must stay as it is beside h_out"
        assert torch.equal(hout.v[real], h1[real]), "h_out must have the bits of h updated in place"
        assert (hout.v[~real] == FILL).all() and torch.equal(skipb.B, Out(M, N - nres, PAD['skip'], init=skip1).B)
    assert not bad, bad


@pytest.mark.parametrize("C,dil", rr.WG_DGRAD)
@pytest.mark.parametrize("prec", PRECS)
def test_wg_dgrad_alone(nv, prec, C, dil):
    c = _dev(rr.make_wg_dgrad(C, dil))
    M, w, rowb, dh0 = rr.WG_M, c['w'], c['rowb'], c['dh0']
    img = _operand(c['img'], PAD['x'])
    d_pre = img[dil:dil + M]
    wt = w.flip(2).permute(1, 2, 0).reshape(C, 6 * C).contiguous()            # WaveGlow._packed's in_wT
    tag, bad = "C=%d dil=%d" % (C, dil), []
    dh, again = Out(M, C, PAD['h'], init=dh0), Out(M, C, PAD['h'], init=dh0)
    nv.wg_dgrad(d_pre, wt, dil, dh.v, True, rowb, prec)
    nv.wg_dgrad(d_pre, wt, dil, again.v, True, rowb, prec)
    _judge("wg_dgrad", tag + " store", prec, {'dh': dh}, lambda mm: rr.wg_dgrad_ref(img, dil, M, w, dil, dh0, True, rowb, prec, mm), bad)
    assert torch.equal(again.B, dh.B), "two calls must give the same bits"
    if prec == 0:                                                 # the restatement is the float64 input gradient of the conv
        hh = torch.zeros(M + 2 * dil, C, dtype=torch.float64, device=DEV, requires_grad=True)
        F.conv1d(hh.t()[None], w.double(), None, dilation=dil, padding=dil).backward(c['img'].double().t()[None])
        real = rowb >= 0
        want = rr.wg_dgrad_ref(img, dil, M, w, dil, dh0, True, rowb, 0)['dh'][0]
        assert rr.rel(want[real], hh.grad[dil:dil + M][real]) < 1e-12
    before = dh.v.clone()
    nv.wg_dgrad(d_pre, wt, dil, dh.v, False, rowb, prec)
    _judge("wg_dgrad", tag + " add", prec, {'dh': dh}, lambda mm: rr.wg_dgrad_ref(img, dil, M, w, dil, before, False, rowb, prec, mm), bad)
    assert not bad, bad


# ---- what the headers promise, bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_vc_linear_bits_do_not_depend_on_the_row_offset_or_the_tile_shape(nv, prec):
    """rowmma.h: "every output's sum runs over K in ascending order", vocos.hip: "a row's sum runs over k in one fixed order
    whatever tile it lies in".  The same 150 rows 37 rows further on sit in other lanes, waves and row tiles; the same 32 weight
    rows are carried by the 4 x 1 waves of a 32-column tile, the 2 x 2 of a 64-column one and the 2 x 2 x (2 x 2) of 128."""
    n, P = 150, 200
    for K in rr.VC_K:
        data, W, b = rr.asym(n, K, 900 + K).to(DEV), rr.asym(128, K, 901 + K, K ** -0.5).to(DEV), rr.asym(1, 128, 902)[0].to(DEV)
        outs = {}
        for off in (3, 40):
            rowb0 = torch.full((P,), -1, dtype=torch.int32, device=DEV)
            rowb0[off:off + n] = 0
            X = torch.zeros(P, K, device=DEV)
            X[off:off + n] = data
            for N in (32, 64, 128):
                out = torch.full((P, N), FILL, device=DEV)
                nv.vc_linear(X, W[:N], b[:N], 'gelu', None, None, out, rowb0, prec)
                outs[(off, N)] = out[off:off + n]
                assert not out[:off].any() and not out[off + n:].any()
        for N in (32, 64, 128):
            assert torch.equal(outs[(3, N)], outs[(40, N)]), "K=%d N=%d: the bits depend on the row offset" % (K, N)
            assert torch.equal(outs[(3, N)][:, :32], outs[(3, 32)]), "K=%d: the bits depend on the tile shape (N=%d)" % (K, N)
        assert outs[(3, 128)].abs().max().item() > 1


@pytest.mark.parametrize("prec", PRECS)
def test_hg_conv_bits_do_not_depend_on_the_row_offset(nv, prec):
    from tacotron2_amd.hifigan import pack_conv
    n, P = 150, 256
    for k, d, Cin, N in rr.HG_CONV:
        data = rr.asym(n, Cin, 910 + k).to(DEV)
        w, b = rr.asym(N, Cin * k, 911 + k, (Cin * k) ** -0.5).view(N, Cin, k).to(DEV), rr.asym(1, N, 912)[0].to(DEV)
        wp, bp = pack_conv(w, b, Cin, N)
        outs = []
        for off in (16, 53):
            rowb0 = torch.full((P,), -1, dtype=torch.int32, device=DEV)
            rowb0[off:off + n] = 0
            X = torch.zeros(P, Cin, device=DEV)
            X[off:off + n] = data
            out = torch.full((P, N), FILL, device=DEV)
            nv.hg_conv(X, wp, bp, k, d, rr.SLOPE, None, out, 1.0, False, rowb0, 1, prec)
            outs.append(out[off:off + n])
            assert not out[:off].any() and not out[off + n:].any()
        assert torch.equal(outs[0], outs[1]), "k=%d d=%d Cin=%d N=%d: the bits depend on the row offset" % (k, d, Cin, N)
        assert outs[0].abs().max().item() > 1
