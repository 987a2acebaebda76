"""float64 restatements of the products that run the shared MFMA tile loop (csrc/rowmma.h): vc_linear (csrc/vocos.hip), hg_conv and
hg_upsample (csrc/hifigan.hip), wg_gated, wg_res_skip and wg_dgrad (csrc/waveglow_layer.hip), in the kernels' own arithmetic.

Plain torch, on whatever device the inputs are on; nothing here calls the code under test.

Precision 0 multiplies the f32 operands as they are.  Precisions 1 and 2 multiply what rm_tile_bf16 multiplies: every operand
value x is split into hi = bf16(x), round to nearest even, and lo = bf16(x - hi); precision 1 adds al wh + ah wl + ah wh (the
al wl term is dropped), precision 2 is ah wh alone.  A product of two bf16 values is exact in f32, so a kernel at precision 1 or 2
differs from `product` of the same precision only by the rounding of its f32 sums: the comparison is as sharp as at precision 0.

Every per-client restatement unfolds the operand the way the kernel's row policy loads it (tap-major K, the activation applied
in float32 BEFORE the rounding), takes the product through `mm` (`product`, or one of F32_PRODUCTS: the same arithmetic in
float32, whose distance from `product` is the yardstick of the GPU tests) and runs the epilogue in the product's dtype.  It
returns {buffer name: (expected, computed)}: the expected contents of the whole view the kernel is given, and the mask of the
elements the kernel computes; every other element must come back bit for bit (zero, or what the buffer held before)."""
import torch


def split(x):
    """hi = bf16(x) (round to nearest even), lo = bf16(x - hi), both as float32; x - hi is exact in float32."""
    x = x.float()
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi, lo


def terms(A, W, prec):
    """The operand pairs (a, w) whose products a K-step adds, in the kernel's order."""
    A, W = A.float(), W.float()
    if prec == 0:
        return [(A, W)]
    ah, al = split(A)
    wh, wl = split(W)
    return [(al, wh), (ah, wl), (ah, wh)] if prec == 1 else [(ah, wh)]


def product(A, W, prec):
    """float64 A [P][K] . W [N][K]^T of the values the kernel multiplies at this precision."""
    return sum(a.double() @ w.double().t() for a, w in terms(A, W, prec))


def product_f32_matmul(A, W, prec):
    """The same arithmetic in float32 through torch's matmul, one product per term."""
    out = None
    for a, w in terms(A, W, prec):
        out = a @ w.t() if out is None else out + a @ w.t()
    return out


def product_f32_ascending(A, W, prec):
    """The same arithmetic in float32 as a plain accumulation over k in ascending order, the terms of a k in the kernel's order."""
    ts = terms(A, W, prec)
    acc = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float32, device=A.device)
    for k in range(A.shape[1]):
        for a, w in ts:
            acc.addcmul_(a[:, k:k + 1], w[:, k].unsqueeze(0))
    return acc


F32_PRODUCTS = (product_f32_matmul, product_f32_ascending)


def product_f32(A, W, prec):
    """Both float32 runs of `product`'s arithmetic: (torch's matmul, ascending k)."""
    return tuple(f(A, W, prec) for f in F32_PRODUCTS)


def rel(a, b):
    """Relative L2 of a against b, in float64."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def unfold(X, offs):
    """The tap-major operand [P][len(offs) C]: column t C + c of row p is X[p + offs[t]][c], zero where that row does not exist."""
    P, C = X.shape
    A = torch.zeros(P, len(offs), C, dtype=X.dtype, device=X.device)
    for t, o in enumerate(offs):
        lo, hi = max(0, -o), min(P, P - o)
        if lo < hi:
            A[lo:hi, t] = X[lo + o:hi + o]
    return A.reshape(P, len(offs) * C)


def lrelu(x, slope):
    """Leaky-ReLU in float32 as the row policy applies it on load (slope None: none)."""
    x = x.float()
    return x if slope is None else torch.where(x > 0, x, x * slope)


def gate_perm(C):
    """Row n of the gate-packed in-layer weights is row gate_perm(C)[n] of the conv's: block 64 q + [0, 32) holds the tanh
    channels 32 q + [0, 32), block 64 q + [32, 64) their sigmoid partners C + 32 q + [0, 32)."""
    return torch.cat([torch.arange(32) + half * C + 32 * q for q in range(C // 32) for half in (0, 1)])


def _real(rowb0, rdiv, P):
    return (torch.repeat_interleave(rowb0, rdiv)[:P] >= 0).unsqueeze(1)


def _all(t):
    return torch.ones(t.shape, dtype=torch.bool, device=t.device)


# ---- Vocos ------------------------------------------------------------------------------------------------------------------
def vc_linear_ref(X, W, bias, epi, gamma, res, rowb0, prec, mm=product):
    """out [P][N] = epi(bias + X W^T) on rows with rowb0 >= 0, zero on the others.  epi None, 'gelu' (exact) or 'residual'
    (res + gamma * .)."""
    v = mm(X, W, prec)
    dt = v.dtype
    if bias is not None:
        v = v + bias.to(dt)
    if epi == 'gelu':
        v = 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752))
    elif epi == 'residual':
        v = res.to(dt) + gamma.to(dt) * v
    real = _real(rowb0, 1, X.shape[0])
    return {'out': (torch.where(real, v, torch.zeros_like(v)), real.expand_as(v))}


# ---- HiFi-GAN ---------------------------------------------------------------------------------------------------------------
def hg_conv_ref(X, w, bias, dil, slope, res, scale, out0, accumulate, rowb0, rdiv, prec, mm=product):
    """Conv1d (weight w [N][Cin][k], dilation dil, 'same' padding) over the row image X [P][Cin] with leaky-ReLU on the
    operand; v = (. + bias (+ res)) * scale, stored or added to out0; zero on rows whose frame rowb0[p // rdiv] is negative."""
    N, Cin, k = w.shape
    A = unfold(lrelu(X, slope), [(t - (k - 1) // 2) * dil for t in range(k)])
    v = mm(A, w.permute(0, 2, 1).reshape(N, k * Cin), prec)
    dt = v.dtype
    if bias is not None:
        v = v + bias.to(dt)
    if res is not None:
        v = v + res.to(dt)
    v = v * scale
    if accumulate:
        v = out0.to(dt) + v
    real = _real(rowb0, rdiv, X.shape[0])
    return {'out': (torch.where(real, v, torch.zeros_like(v)), real.expand_as(v))}


def hg_upsample_ref(X, w, bias, u, slope, rowb0, rdiv, prec, mm=product):
    """ConvTranspose1d (weight w [Cin][N][ku], stride u, padding (ku - u) / 2) over the row image X [P][Cin] in its polyphase
    form: output row u m + ph, q = ph + pad, adds the taps kk = q % u + u j of the input rows m + q // u - j."""
    Cin, N, ku = w.shape
    pad, taps, P = (ku - u) // 2, ku // u, X.shape[0]
    Xa = lrelu(X, slope)
    out = None
    for ph in range(u):
        q = ph + pad
        A = unfold(Xa, [q // u - j for j in range(taps)])
        Wp = torch.cat([w[:, :, q % u + u * j].t() for j in range(taps)], 1)
        v = mm(A, Wp, prec)
        if bias is not None:
            v = v + bias.to(v.dtype)
        if out is None:
            out = torch.zeros(P * u, N, dtype=v.dtype, device=v.device)
        out[ph::u] = v
    real = _real(rowb0, rdiv * u, P * u)
    return {'out': (torch.where(real, out, torch.zeros_like(out)), real.expand_as(out))}


# ---- WaveGlow ---------------------------------------------------------------------------------------------------------------
def wg_in_product(img, r0, M, w, dil, prec, mm=product):
    """Rows r0 .. r0 + M - 1 of the kernel-3 dilated conv1d (weight w [2C][C][3], channel order) over the row image img."""
    A = unfold(img, [-dil, 0, dil])[r0:r0 + M]
    return mm(A, w.permute(0, 2, 1).reshape(w.shape[0], 3 * w.shape[1]), prec)


def wg_gated_ref(img, r0, M, w, bias, dil, cnd, prec, mm=product):
    """Mode 0: acts = tanh(t) sigmoid(s) with [t | s] = conv + bias + cnd [M][2C], and gate = [tanh(t) | sigmoid(s)]."""
    pre = wg_in_product(img, r0, M, w, dil, prec, mm)
    pre = (pre + bias.to(pre.dtype)) + cnd.to(pre.dtype)
    C = w.shape[1]
    t, s = torch.tanh(pre[:, :C]), torch.sigmoid(pre[:, C:])
    gate = torch.cat([t, s], 1)
    return {'acts': (t * s, _all(t)), 'gate': (gate, _all(gate))}


def wg_res_skip_ref(acts, W, bias, h0, skip0, skip_store, rowb, prec, mm=product, h_out0=None):
    """Mode 1: v = acts W^T + bias [M][N]; the first nres = h0's width columns are added to h on rows with rowb >= 0 (h0 None:
    no residual half), the others are stored in or added to skip on every row.  h_out0: the sums go there, h stays as it is."""
    v = mm(acts, W, prec)
    dt = v.dtype
    v = v + bias.to(dt)
    nres = 0 if h0 is None else h0.shape[1]
    out = {}
    if nres:
        real = (rowb[:acts.shape[0]] >= 0).unsqueeze(1)
        new = torch.where(real, h0.to(dt) + v[:, :nres], (h0 if h_out0 is None else h_out0).to(dt))
        if h_out0 is None:
            out['h'] = (new, real.expand_as(new))
        else:
            out['h'] = (h0.to(dt), ~_all(h0))
            out['h_out'] = (new, real.expand_as(new))
    sk = v[:, nres:] if skip_store else skip0.to(dt) + v[:, nres:]
    out['skip'] = (sk, _all(sk))
    return out


def wg_dgrad_ref(img, r0, M, w, dil, dh0, store, rowb, prec, mm=product):
    """Mode 2: the input gradient of the in-layer conv1d (weight w [2C][C][3]) from the image img of d_pre [.][2C]:
    dh[m][c] (+)= sum over tap, n of d_pre[m - (tap - 1) dil][n] w[n][c][tap] on rows with rowb >= 0."""
    A = unfold(img, [-dil, 0, dil])[r0:r0 + M]
    Wt = torch.cat([w[:, :, 2 - t].t() for t in range(3)], 1)                  # [C][3 * 2C], the taps mirrored
    v = mm(A, Wt, prec)
    dt = v.dtype
    real = (rowb[:M] >= 0).unsqueeze(1)
    new = torch.where(real, v if store else dh0.to(dt) + v, dh0.to(dt))
    return {'dh': (new, real.expand_as(new))}


# ---- the cases and the data of the kernel-alone tests (tests/test_rowmma_ref_cpu.py, tests/test_zz17_rowmma_gpu.py) ---------------
VC_K = (32, 64, 96)                                   # 1, 2 and 3 K-steps of the bf16 family
VC_N = (32, 64, 128, 160, 192)                        # column tiles of 32, 64, 128, 32 and 64
VC_LENS = ([1], [122], [123], [3, 1, 140])            # P = 7, 128 exactly, 129, 156 packed rows
HG_CONV = [(3, 1, 32, 32), (3, 3, 64, 64), (5, 6, 64, 96), (7, 5, 128, 128), (11, 1, 96, 64), (1, 1, 32, 160)]   # k, d, Cin, N
HG_CONV_PLAN = ([3, 1, 2], 2, 16)                     # lens, H, S: 224 rows, halos of 32 rows >= the widest half-window 15
HG_UP = [(64, 32, 4, 2), (32, 32, 16, 8), (96, 64, 12, 4), (64, 64, 6, 2), (32, 64, 4, 4)]                      # ci, co, ku, u
HG_UP_PLAN = ([5, 1, 3], 1, 12)                       # 156 input rows
WG_GATED = [(C, dil, M) for C in (64, 128) for dil in (1, 8) for M in (5, 128, 200)]
WG_RES_SKIP = [(64, 128, 64), (64, 64, 0), (128, 256, 128)]                                                     # C, N, nres
WG_DGRAD = [(64, 1), (64, 8), (128, 4)]                                                                         # C, dil
WG_M = 133                                            # two row tiles, the second of five rows
SLOPE = 0.1


def asym(rows, cols, seed, scale=1.0):
    """Random values with row i scaled by 1 + i / rows and column k by 1 + k / cols, so that no transposed, permuted or
    shifted fragment reproduces them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g) * scale
    return x * (1 + torch.arange(rows).float() / rows).unsqueeze(1) * (1 + torch.arange(cols).float() / cols).unsqueeze(0)


def plan(lens, H):
    """(rowb0, offsets, P0) of a frame-level row space: H halo rows (rowb0 -1) before, between and after the utterances."""
    rowb, offs, pos = [torch.full((H,), -1, dtype=torch.int32)], [], H
    for b, n in enumerate(lens):
        offs.append(pos)
        rowb += [torch.full((n,), b, dtype=torch.int32), torch.full((H,), -1, dtype=torch.int32)]
        pos += n + H
    return torch.cat(rowb), offs, pos


def _image(rowb0, S, C, seed, scale=1.0):
    """A row image [P0 S][C]: asymmetric random real rows, zero halo rows."""
    P = rowb0.numel() * S
    return asym(P, C, seed, scale) * (torch.repeat_interleave(rowb0, S) >= 0).float().unsqueeze(1)


def _rowb(M):
    """A row map of M rows with negative rows inside the range: two runs of three, and the last row."""
    rowb = torch.zeros(M, dtype=torch.int32)
    for o in (M // 3, 2 * M // 3):
        rowb[o:o + 3] = -1
    rowb[M - 1] = -1
    return rowb


def make_vc(K, N, lens, seed=0):
    from tacotron2_amd.vocos import Vocos
    import vocos_ref as vr
    rowb0, _, _, offs, P = Vocos(**vr.CONFIGS['small']).packed_plan(lens)
    s = 1000 * seed + 7 * K + N + len(lens)
    return dict(P=P, offs=offs, lens=lens, rowb0=rowb0, X=_image(rowb0, 1, K, s), W=asym(N, K, s + 1, K ** -0.5),
                bias=torch.linspace(-10.0, 10.0, N), gamma=asym(1, N, s + 2, 0.5)[0], res=_image(rowb0, 1, N, s + 3))


def make_hg_conv(k, d, Cin, N, seed=0):
    lens, H, S = HG_CONV_PLAN
    rowb0, offs, P0 = plan(lens, H)
    s = 1000 * seed + 100 * k + 10 * d + Cin + N
    w = asym(N, Cin * k, s + 1, (Cin * k) ** -0.5).view(N, Cin, k)
    return dict(P=P0 * S, S=S, offs=offs, lens=lens, rowb0=rowb0, X=_image(rowb0, S, Cin, s), w=w,
                bias=asym(1, N, s + 2)[0], res=_image(rowb0, S, N, s + 3))


def make_hg_up(ci, co, ku, u, seed=0):
    lens, H, S = HG_UP_PLAN
    rowb0, offs, P0 = plan(lens, H)
    s = 1000 * seed + 100 * ku + 10 * u + ci + co
    w = asym(ci, co * ku, s + 1, (ci * ku / u) ** -0.5).view(ci, co, ku)
    return dict(P=P0 * S, S=S, offs=offs, lens=lens, rowb0=rowb0, X=_image(rowb0, S, ci, s), w=w, bias=asym(1, co, s + 2)[0])


def make_wg_in(C, seed):
    """The in-layer conv1d of WaveGlow's WN: weight [2C][C][3] and bias [2C], channel order."""
    return asym(2 * C, 3 * C, seed, (3 * C) ** -0.5).view(2 * C, C, 3), asym(1, 2 * C, seed + 1, 0.5)[0]


def make_wg_gated(C, dil, M, seed=0):
    s = 1000 * seed + 10 * C + dil + M
    img = torch.zeros(M + 2 * dil, C)
    img[dil:dil + M] = asym(M, C, s)
    w, bias = make_wg_in(C, s + 1)
    return dict(img=img, w=w, bias=bias, cnd=asym(M, 2 * C, s + 3, 0.5))


def make_wg_res_skip(C, N, nres, M=WG_M, seed=0):
    s = 1000 * seed + 10 * C + N + nres
    return dict(acts=asym(M, C, s, 0.5), W=asym(N, C, s + 1, C ** -0.5), bias=asym(1, N, s + 2, 0.5)[0],
                h0=asym(M, nres, s + 3) if nres else None, skip0=asym(M, N - nres, s + 4), rowb=_rowb(M))


def make_wg_dgrad(C, dil, M=WG_M, seed=0):
    s = 1000 * seed + 10 * C + dil
    rowb = _rowb(M)
    img = torch.zeros(M + 2 * dil, 2 * C)
    img[dil:dil + M] = asym(M, 2 * C, s) * (rowb >= 0).float().unsqueeze(1)     # d_pre is zero on the halo rows
    w, _ = make_wg_in(C, s + 1)
    return dict(img=img, w=w, dh0=asym(M, C, s + 3), rowb=rowb)
