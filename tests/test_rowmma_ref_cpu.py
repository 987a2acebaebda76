"""tests/rowmma_ref.py, the float64 restatements behind the kernel-alone tests of the shared MFMA tile loop (csrc/rowmma.h), proved
here on the CPU: at precision 0 each equals torch's own float64 operator on the shapes tests/test_zz17_rowmma_gpu.py runs; the
gate packing and the bf16 split equal the ones in force; and the limit of the GPU tests (10 x the error of the float32 runs of
the same arithmetic) is sharp enough that every single-fragment mistake a tile loop can make misses it by at least 100 x."""
import pytest
import torch
import torch.nn.functional as F

import rowmma_ref as rr

EXACT = 1e-12
PRECS = (0, 1, 2)


def _utts(c):
    """(first row, rows) of every utterance of a packed image, in image rows."""
    S = c.get('S', 1)
    return [(o * S, n * S) for o, n in zip(c['offs'], c['lens'])]


# ---- precision 0 is torch's float64 operator -------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", rr.VC_LENS)
def test_vc_linear_ref_is_f_linear(lens):
    for K in rr.VC_K:
        for N in rr.VC_N:
            c = rr.make_vc(K, N, lens)
            real = c['rowb0'] >= 0
            assert c['P'] == sum(lens) + 3 * (len(lens) + 1) and int(real.sum()) == sum(lens)
            pre = F.linear(c['X'].double(), c['W'].double(), c['bias'].double())
            assert pre[real].min() < -8 and pre[real].max() > 8, "the GELU inputs must span both tails"
            want = {None: pre, 'gelu': F.gelu(pre), 'residual': c['res'].double() + c['gamma'].double() * pre}
            for epi in (None, 'gelu', 'residual'):
                got, mask = rr.vc_linear_ref(c['X'], c['W'], c['bias'], epi, c['gamma'], c['res'], c['rowb0'], 0)['out']
                assert got.dtype == torch.float64 and torch.equal(mask, real.unsqueeze(1).expand_as(got))
                assert not got[~real].any() and rr.rel(got[real], want[epi][real]) < EXACT, (K, N, epi)


@pytest.mark.parametrize("k,d,Cin,N", rr.HG_CONV)
def test_hg_conv_ref_is_f_conv1d(k, d, Cin, N):
    c = rr.make_hg_conv(k, d, Cin, N)
    assert (k - 1) // 2 * d <= 2 * c['S'], "the halo must cover the half-window"
    store = rr.hg_conv_ref(c['X'], c['w'], c['bias'], d, rr.SLOPE, None, 1.0, None, False, c['rowb0'], c['S'], 0)['out'][0]
    fused = rr.hg_conv_ref(c['X'], c['w'], c['bias'], d, rr.SLOPE, c['res'], 0.5, store, True, c['rowb0'], c['S'], 0)['out'][0]
    real = torch.repeat_interleave(c['rowb0'], c['S']) >= 0
    assert not store[~real].any() and not fused[~real].any() and int(real.sum()) == sum(c['lens']) * c['S']
    for o, n in _utts(c):
        x = F.leaky_relu(c['X'][o:o + n], rr.SLOPE).double().t()[None]
        want = F.conv1d(x, c['w'].double(), c['bias'].double(), dilation=d, padding=d * (k - 1) // 2)[0].t()
        assert rr.rel(store[o:o + n], want) < EXACT
        assert rr.rel(fused[o:o + n], want + 0.5 * (want + c['res'][o:o + n].double())) < EXACT


@pytest.mark.parametrize("ci,co,ku,u", rr.HG_UP)
def test_hg_upsample_ref_is_f_conv_transpose1d(ci, co, ku, u):
    c = rr.make_hg_up(ci, co, ku, u)
    got, mask = rr.hg_upsample_ref(c['X'], c['w'], c['bias'], u, rr.SLOPE, c['rowb0'], c['S'], 0)['out']
    assert got.shape == (c['P'] * u, co) and not got[~mask].any()
    for o, n in _utts(c):
        x = F.leaky_relu(c['X'][o:o + n], rr.SLOPE).double().t()[None]
        want = F.conv_transpose1d(x, c['w'].double(), c['bias'].double(), stride=u, padding=(ku - u) // 2)[0].t()
        assert mask[o * u:(o + n) * u].all() and rr.rel(got[o * u:(o + n) * u], want) < EXACT
        for ph in range(u):
            assert rr.rel(got[o * u + ph:(o + n) * u:u], want[ph::u]) < EXACT, ph


@pytest.mark.parametrize("C,dil,M", rr.WG_GATED)
def test_wg_gated_ref_is_the_gated_conv1d(C, dil, M):
    c = rr.make_wg_gated(C, dil, M)
    out = rr.wg_gated_ref(c['img'], dil, M, c['w'], c['bias'], dil, c['cnd'], 0)
    x = c['img'][dil:dil + M].double().t()[None]
    pre = F.conv1d(x, c['w'].double(), c['bias'].double(), dilation=dil, padding=dil)[0].t() + c['cnd'].double()
    t, s = torch.tanh(pre[:, :C]), torch.sigmoid(pre[:, C:])
    assert rr.rel(out['acts'][0], t * s) < EXACT and rr.rel(out['gate'][0], torch.cat([t, s], 1)) < EXACT
    assert out['acts'][1].all() and out['gate'][1].all()


@pytest.mark.parametrize("C,N,nres", rr.WG_RES_SKIP)
def test_wg_res_skip_ref_is_f_linear(C, N, nres):
    c = rr.make_wg_res_skip(C, N, nres)
    real = c['rowb'] >= 0
    assert 0 < int((~real).sum()) < 10 and not real[-1] and real[0]
    v = F.linear(c['acts'].double(), c['W'].double(), c['bias'].double())
    for store in (True, False):
        out = rr.wg_res_skip_ref(c['acts'], c['W'], c['bias'], c['h0'], c['skip0'], store, c['rowb'], 0)
        want = v[:, nres:] if store else c['skip0'].double() + v[:, nres:]
        assert rr.rel(out['skip'][0], want) < EXACT and out['skip'][1].all()
        if nres:
            h, mask = out['h']
            assert torch.equal(h[~real], c['h0'][~real].double()) and torch.equal(mask[:, 0], real)
            assert rr.rel(h[real], (c['h0'].double() + v[:, :nres])[real]) < EXACT
    if nres:
        side = torch.full_like(c['h0'], 7.0)
        out = rr.wg_res_skip_ref(c['acts'], c['W'], c['bias'], c['h0'], c['skip0'], True, c['rowb'], 0, h_out0=side)
        assert torch.equal(out['h'][0], c['h0'].double()) and not out['h'][1].any()
        assert torch.equal(out['h_out'][0][real], h[real]) and (out['h_out'][0][~real] == 7.0).all()


@pytest.mark.parametrize("C,dil", rr.WG_DGRAD)
def test_wg_dgrad_ref_is_the_input_gradient_of_the_conv1d(C, dil):
    c = rr.make_wg_dgrad(C, dil)
    M = rr.WG_M
    real = c['rowb'] >= 0
    h = torch.zeros(M + 2 * dil, C, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(h.t()[None], c['w'].double(), None, dilation=dil, padding=dil)
    y.backward(c['img'].double().t()[None])
    want = h.grad[dil:dil + M]
    store, _ = rr.wg_dgrad_ref(c['img'], dil, M, c['w'], dil, c['dh0'], True, c['rowb'], 0)['dh']
    add, _ = rr.wg_dgrad_ref(c['img'], dil, M, c['w'], dil, c['dh0'], False, c['rowb'], 0)['dh']
    assert rr.rel(store[real], want[real]) < EXACT and rr.rel(add[real], (c['dh0'].double() + want)[real]) < EXACT
    assert torch.equal(store[~real], c['dh0'][~real].double()) and torch.equal(add[~real], c['dh0'][~real].double())


# ---- the packing and the split in force -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 128])
def test_gate_perm_is_the_packing_of_waveglow(C):
    from tacotron2_amd.waveglow import WaveGlow
    torch.manual_seed(C)
    wg = WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=C, kernel_size=3))
    f = wg._packed(torch.device("cpu"))['flows'][0]
    perm = rr.gate_perm(C)
    assert sorted(perm.tolist()) == list(range(2 * C))
    for i in range(2):
        conv = wg.WN[0].in_layers[i]
        w = conv.weight.detach().float()
        assert torch.equal(f['in_w'][i], w.permute(0, 2, 1).reshape(2 * C, 3 * C)[perm])
        assert torch.equal(f['in_b'][i], conv.bias.detach().float()[perm])
        # and the data gradient's operand is the one wg_dgrad_ref builds
        assert torch.equal(f['in_wT'][i], torch.cat([w[:, :, 2 - t].t() for t in range(3)], 1))


def test_split_is_the_split_of_the_bf16x3_images():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(64, 96, generator=g) * torch.logspace(-3, 2, 96).unsqueeze(0)
    hi, lo = rr.split(x)
    assert torch.equal(hi, x.bfloat16().float()) and torch.equal(lo.bfloat16().float(), lo)
    assert ((hi.double() + lo.double() - x.double()).abs() <= 2.0 ** -17 * x.double().abs()).all()
    # tests/test_kernels_gpu.py's restatement of t2amd_split_bf16x3_f32: per 16 k, 16 hi then 16 lo
    import test_kernels_gpu as tk
    img = tk.split_image_ref(x).float().reshape(64, 6, 2, 16)
    assert torch.equal(img[:, :, 0].reshape(64, 96), hi) and torch.equal(img[:, :, 1].reshape(64, 96), lo)


# ---- every mistake of one fragment misses the limit by 100 x ------------------------------------------------------------------
def _limit(fn):
    """10 x e32 of a case, e32 the larger distance of its two float32 runs from the float64 one (over every buffer)."""
    want = fn(rr.product)
    e32 = max(_dist(fn(mm), want) for mm in rr.F32_PRODUCTS)
    assert e32 > 0
    return want, 10 * e32


def _dist(got, want):
    return max(rr.rel(got[k][0], want[k][0]) for k in want)


def _mm_without_al_wh(A, W, prec):
    assert prec == 1
    return sum(a.double() @ w.double().t() for a, w in rr.terms(A, W, 1)[1:])


def _mm_truncated(A, W, prec):
    assert prec == 2
    chop = lambda x: (x.float().view(torch.int32) & -65536).view(torch.float32).double()    # noqa: E731
    return chop(A) @ chop(W).t()


def _mm_short(A, W, prec):
    step = 16 if prec == 0 else 32
    return rr.product(A[:, :-step], W[:, :-step], prec)


@pytest.mark.parametrize("prec", PRECS)
def test_a_wrong_conv_misses_the_limit_by_100x(prec):
    k, d, Cin, N = 5, 6, 64, 96
    c = rr.make_hg_conv(k, d, Cin, N)
    prev = rr.asym(c['P'], N, 77)

    def run(mm, X=c['X'], w=c['w'], bias=c['bias'], dil=d, slope=rr.SLOPE, rowb0=c['rowb0']):
        return rr.hg_conv_ref(X, w, bias, dil, slope, c['res'], 0.5, prev, True, rowb0, c['S'], prec, mm)

    want, limit = _limit(run)
    wrong = {
        'taps in reverse order': run(rr.product, w=c['w'].flip(2)),
        'dilation off by one': run(rr.product, dil=d + 1),
        'every tap shifted by one row': run(rr.product, X=torch.cat([torch.zeros(1, Cin), c['X'][:-1]])),
        'the last K-step missing': run(_mm_short),
        'leaky-ReLU omitted': run(rr.product, slope=None),
        'bias taken from column n + 32': run(rr.product, bias=c['bias'].roll(-32)),
        'residual added on halo rows': run(rr.product, rowb0=torch.zeros_like(c['rowb0'])),
    }
    if prec == 1:
        wrong['the al wh term dropped'] = run(_mm_without_al_wh)
    if prec == 2:
        wrong['operands truncated instead of rounded'] = run(_mm_truncated)
    for name, got in wrong.items():
        miss = _dist(got, want) / limit
        print("precision %d, conv, %s: %.3g x the limit %.3g" % (prec, name, miss, limit))
        assert miss >= 100, (name, miss)


@pytest.mark.parametrize("prec", PRECS)
def test_a_wrong_waveglow_product_misses_the_limit_by_100x(prec):
    C, dil, M = 128, 8, 200
    c = rr.make_wg_gated(C, dil, M)

    def gated(mm, img=c['img'], w=c['w'], bias=c['bias'], cnd=c['cnd'], dil_=dil):
        return rr.wg_gated_ref(img, dil, M, w, bias, dil_, cnd, prec, mm)

    want, limit = _limit(gated)
    swap = lambda t, dim: t.roll(C, dim)                                                      # noqa: E731
    wrong = {
        'tanh and sigmoid partners swapped': gated(rr.product, w=swap(c['w'], 0), bias=swap(c['bias'], 0), cnd=swap(c['cnd'], 1)),
        'bias taken from column n + 32': gated(rr.product, bias=c['bias'].roll(-32)),
        'taps in reverse order': gated(rr.product, w=c['w'].flip(2)),
        'dilation off by one': gated(rr.product, dil_=dil + 1),
        'every tap shifted by one row': gated(rr.product, img=torch.cat([torch.zeros(1, C), c['img'][:-1]])),
        'the last K-step missing': gated(_mm_short),
    }
    if prec == 1:
        wrong['the al wh term dropped'] = gated(_mm_without_al_wh)
    if prec == 2:
        wrong['operands truncated instead of rounded'] = gated(_mm_truncated)
    for name, got in wrong.items():
        miss = _dist(got, want) / limit
        print("precision %d, gated, %s: %.3g x the limit %.3g" % (prec, name, miss, limit))
        assert miss >= 100, (name, miss)

    r = rr.make_wg_res_skip(128, 256, 128)

    def res_skip(mm, rowb=r['rowb'], bias=r['bias']):
        return rr.wg_res_skip_ref(r['acts'], r['W'], bias, r['h0'], r['skip0'], False, rowb, prec, mm)

    want, limit = _limit(res_skip)
    wrong = {'residual added on halo rows': res_skip(rr.product, rowb=torch.zeros_like(r['rowb'])),
             'bias taken from column n + 32': res_skip(rr.product, bias=r['bias'].roll(-32)),
             'the last K-step missing': res_skip(_mm_short)}
    for name, got in wrong.items():
        miss = _dist(got, want) / limit
        print("precision %d, residual / skip, %s: %.3g x the limit %.3g" % (prec, name, miss, limit))
        assert miss >= 100, (name, miss)
