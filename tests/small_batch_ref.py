"""The small-batch (B <= 8) matrix-vector kernels of csrc/gemv.hip ("Tolerance of the small-batch kernels")
restated in numpy, with the cases the CPU and the GPU tests share.

``lstm_step64`` / ``linear64`` are the definition in float64:
  LSTM step   X = the segments side by side (an absent one is zeros), pre = X W^T + gin + bias, rows g H + j in the gate order
              i, f, g, o; c = f c_prev + i g; h = o tanh(c) keep keep_scale; a row with t >= lens[b] is zero gates, c and h;
  linear      act(X W^T + bias) keep keep_scale, act 0 the identity and 1 the ReLU.
``lstm_step32`` / ``linear32`` are the same formulas in float32 with the product as one fmaf chain over k ascending; they exist
to set the tolerance max(4 x the float32 restatement's own largest error, 8 2^-24 max(1, largest |value| in float64))
(``fft_block_ref.error`` / ``allowed``).  Under bf16 weights the bf16-rounded weights ARE the case's weights, in both
restatements: rounding them is no error of the kernel's.

The runners lay every tensor out inside a wider buffer of NaN (``Slab``): every row stride exceeds its width, every base is
16 bytes into its buffer, and after the call everything around an output must still be NaN."""
import functools

import numpy as np
import torch

import fft_block_ref as fr

F32 = np.float32
NAN = float("nan")
EVERY_B = tuple(range(1, 9))
LOOP_EDGES = (1, 63, 64, 65, 128, 129, 192, 193, 257)          # Kn: 16-byte units per weight row (4 k in f32, 8 k in bf16)
FORMATS = ("f32", "bf16")
LIN_N, LIN_B, LIN_K = (1, 15, 16, 17, 81), (1, 4, 7, 8), (4, 80, 256, 260, 516)
KEEP_RATE, KEEP_DROP = 0.9, 0.1
# float32 saturation (a correctly rounded 1 + e is 1 for e <= 2^-25; expf overflows to inf beyond 88.73): a sigmoid gate is
# exactly 1 from a pre-activation of 18 (e^-18 = 1.5e-8 < 2^-25 = 3.0e-8) and exactly +0 below -90; tanh is exactly +-1 from
# |x| = 10 (1 - tanh 10 = 4.1e-9 < 2^-25)
SIGMOID_ONE, SIGMOID_ZERO, TANH_ONE = 18.0, -90.0, 10.0
PLANTED = (100.0, -100.0, 20.0, -20.0)                          # the bias of units 0 .. 3 of every gate in a planted case


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


# ---- the definition, in either precision -------------------------------------------------------------------------------------------
def _sigmoid(x):
    with np.errstate(over="ignore"):
        return (1 / (1 + np.exp(-x))).astype(x.dtype)


def _cat(xs, widths, B, dtype):
    return np.concatenate([np.zeros((B, w), dtype) if x is None else np.asarray(x, dtype) for x, w in zip(xs, widths)], axis=1)


def _product(X, W, dtype):
    return fr.chain(X, W) if dtype == F32 else X @ np.asarray(W, dtype).T


def _lstm_step(dtype, xs, widths, W, H, B, gin, bias, c_prev, keep, keep_scale, lens, t):
    pre = _product(_cat(xs, widths, B, dtype), W, dtype)
    if gin is not None:
        pre = pre + np.asarray(gin, dtype)
    if bias is not None:
        pre = pre + np.asarray(bias, dtype)
    i, f, o = (_sigmoid(pre[:, g * H:(g + 1) * H]) for g in (0, 1, 3))
    g = np.tanh(pre[:, 2 * H:3 * H])
    c = i * g if c_prev is None else f * np.asarray(c_prev, dtype) + i * g
    h = o * np.tanh(c)
    if keep is not None:
        h = h * np.asarray(keep, dtype) * dtype(keep_scale)
    gates = np.concatenate((i, f, g, o), axis=1)
    if lens is not None:
        live = (t < np.asarray(lens))[:, None]
        gates, c, h = (np.where(live, a, dtype(0)) for a in (gates, c, h))
    return dict(gates=gates.astype(dtype), c=c.astype(dtype), h=h.astype(dtype), pre=pre)


def lstm_step64(xs, widths, W, H, B, gin=None, bias=None, c_prev=None, keep=None, keep_scale=1.0, lens=None, t=0):
    return _lstm_step(np.float64, xs, widths, W, H, B, gin, bias, c_prev, keep, keep_scale, lens, t)


def lstm_step32(xs, widths, W, H, B, gin=None, bias=None, c_prev=None, keep=None, keep_scale=1.0, lens=None, t=0):
    return _lstm_step(F32, xs, widths, W, H, B, gin, bias, c_prev, keep, keep_scale, lens, t)


def _linear(dtype, X, W, bias, act, keep, keep_scale):
    y = _product(np.asarray(X, dtype), W, dtype)
    if bias is not None:
        y = y + np.asarray(bias, dtype)
    if act == 1:
        y = np.maximum(y, dtype(0))
    if keep is not None:
        y = y * np.asarray(keep, dtype) * dtype(keep_scale)
    return y.astype(dtype)


def linear64(X, W, bias=None, act=0, keep=None, keep_scale=1.0):
    return _linear(np.float64, X, W, bias, act, keep, keep_scale)


def linear32(X, W, bias=None, act=0, keep=None, keep_scale=1.0):
    return _linear(F32, X, W, bias, act, keep, keep_scale)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def bf16_round(w):
    """float32 values that bf16 holds exactly (round to nearest even, as torch casts)."""
    return torch.from_numpy(np.ascontiguousarray(w, F32)).bfloat16().float().numpy()


def keep_scale():
    from tacotron2_amd import native
    return native.scale_for(KEEP_DROP)


def split3(K):
    """K as three positive multiples of 4 that add up to it; as two or one where K is 8 or 4."""
    if K < 12:
        return (K,) if K < 8 else (4, K - 4)
    a = max(4, K // 5 // 4 * 4)
    b = max(4, K // 3 // 4 * 4)
    return (a, b, K - a - b)


def edge_widths(Kn, fmt):
    """The loop-edge case's segments: K = 4 Kn (f32 weights) or 8 Kn (bf16 weights); under bf16 weights at Kn = 65 and 129 the
    first two widths are 12 and 20, both 4 mod 8, so that an eight-k unit of the weight row straddles two segments."""
    K = (8 if fmt == "bf16" else 4) * Kn
    if fmt == "bf16" and Kn in (65, 129):
        return (12, 20, K - 32)
    return split3(K)


@functools.lru_cache(maxsize=None)
def lstm_case(B, H, widths, fmt="f32", absent=(), gin=True, bias=True, c_prev=True, keep=False, lens=None, t=0, planted=False,
              quiet=1.0, seed=0):
    """One LSTM step with its float64 and float32 restatements.  ``absent``: positions of segments passed as NULL; ``lens``: a
    tuple of B lengths; ``planted``: PLANTED on the bias of units 0 .. 3 of every gate, the rest of the pre-activation scaled by
    ``quiet``.  Cached: the tests share one case and must leave it unchanged."""
    K = sum(widths)
    r = np.random.default_rng(seed * 7919 + B * 131 + H * 17 + K + len(absent))
    W = (r.standard_normal((4 * H, K)) * (quiet / np.sqrt(K))).astype(F32)
    if fmt == "bf16":
        W = bf16_round(W)
    case = dict(B=B, H=H, widths=tuple(widths), fmt=fmt, W=W, t=t, keep_scale=1.0,
                xs=[None if i in absent else r.standard_normal((B, w)).astype(F32) for i, w in enumerate(widths)],
                gin=(quiet * 0.5 * r.standard_normal((B, 4 * H))).astype(F32) if gin else None,
                bias=(quiet * 0.5 * r.standard_normal(4 * H)).astype(F32) if bias else None,
                c_prev=r.standard_normal((B, H)).astype(F32) if c_prev else None,
                keep=(r.random((B, H)) < KEEP_RATE).astype(np.uint8) if keep else None,
                lens=None if lens is None else np.asarray(lens, np.int32))
    if keep:
        case["keep_scale"] = keep_scale()
    if planted:
        for g in range(4):
            case["bias"][g * H:g * H + 4] = PLANTED
    args = (case["xs"], widths, W, H, B, case["gin"], case["bias"], case["c_prev"], case["keep"], case["keep_scale"], case["lens"], t)
    case["f64"], case["f32"] = lstm_step64(*args), lstm_step32(*args)
    for a in case["f64"].values():
        a.setflags(write=False)
    return case


def lstm_row(case, b):
    """Row b of the case as a B = 1 case of its own (no restatements: it is compared with the batch's bits)."""
    cut = lambda a: None if a is None else np.ascontiguousarray(a[b:b + 1])          # noqa: E731
    return dict(case, B=1, xs=[cut(x) for x in case["xs"]], gin=cut(case["gin"]), c_prev=cut(case["c_prev"]),
                keep=cut(case["keep"]), lens=cut(case["lens"]))


@functools.lru_cache(maxsize=None)
def linear_case(B, N, K, act=0, bias=True, keep=False, seed=0):
    r = np.random.default_rng(seed * 104729 + B * 131 + N * 17 + K)
    case = dict(B=B, N=N, K=K, act=act, keep_scale=keep_scale() if keep else 1.0,
                X=r.standard_normal((B, K)).astype(F32), W=(r.standard_normal((N, K)) / np.sqrt(K)).astype(F32),
                bias=r.standard_normal(N).astype(F32) if bias else None,
                keep=(r.random((B, N)) < KEEP_RATE).astype(np.uint8) if keep else None)
    args = (case["X"], case["W"], case["bias"], act, case["keep"], case["keep_scale"])
    case["f64"], case["f32"] = linear64(*args), linear32(*args)
    case["f64"].setflags(write=False)
    return case


# ---- layout ----------------------------------------------------------------------------------------------------------------------
class Slab:
    """A (rows, width) tensor inside a longer buffer: ``lead`` elements in front, a row stride of width + pad, the last row's
    pad (or ``lead`` elements, where pad is 0) behind it, all of it ``fill`` (NaN) around the data."""

    def __init__(self, dev, rows=0, width=0, data=None, pad=4, lead=4, dtype=torch.float32, fill=NAN):
        if data is not None:
            data = np.asarray(data)
            rows, width = data.shape
        self.rows, self.width, self.ld, self.lead = rows, width, width + pad, lead
        host = torch.full((lead + rows * self.ld + (0 if pad else lead),), fill, dtype=dtype)
        if data is not None:
            self._of(host).copy_(torch.from_numpy(np.ascontiguousarray(data)))
        self.whole = host.to(dev)
        self.view = self._of(self.whole)

    def _of(self, whole):
        return whole[self.lead:self.lead + self.rows * self.ld].view(self.rows, self.ld)[:, :self.width]

    def numpy(self):
        return self.view.float().cpu().numpy()

    def intact(self):
        """Everything around the data is still NaN."""
        host = self.whole.cpu()
        outside = torch.ones(host.numel(), dtype=torch.bool)
        self._of(outside).fill_(False)
        return bool(torch.isnan(host[outside]).all())


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def run_lstm(case, dev, small=True, gates=True, pad=1, w_lead=None, bf16=None):
    """native.lstm_step_fwd on the case -> dict of numpy gates (or None), c, h.  ``pad`` scales the slack of every row stride
    (0: plain contiguous tensors); ``w_lead``: elements in front of the weights (default 16 bytes); ``bf16``: the value passed
    on, by default 2 under bf16 weights."""
    from tacotron2_amd import native
    B, H, w16 = case["B"], case["H"], case["fmt"] == "bf16"
    slab = lambda a, p, **kw: None if a is None else Slab(dev, data=a, pad=p * pad, **kw)          # noqa: E731
    xs = [slab(x, 4 + 4 * (i % 2)) for i, x in enumerate(case["xs"])]
    W = Slab(dev, data=case["W"], pad=0, lead=(8 if w16 else 4) if w_lead is None else w_lead,
             dtype=torch.bfloat16 if w16 else torch.float32)
    gin, c_prev = slab(case["gin"], 5), slab(case["c_prev"], 1)
    bias = slab(None if case["bias"] is None else case["bias"][None], 3)
    keep = slab(case["keep"], 3, dtype=torch.uint8, fill=1)
    lens = None if case["lens"] is None else torch.from_numpy(case["lens"]).to(dev)
    out = dict(gates=Slab(dev, B, 4 * H, pad=3 * pad) if gates else None, c=Slab(dev, B, H, pad=pad), h=Slab(dev, B, H, pad=2 * pad))
    v = lambda s: None if s is None else s.view                                        # noqa: E731
    try:
        native.lstm_step_fwd([v(x) for x in xs], list(case["widths"]), W.view, H, B, v(out["gates"]), out["c"].view, out["h"].view,
                             gin=v(gin), bias=None if bias is None else bias.view[0], c_prev=v(c_prev), keep=v(keep),
                             keep_scale=case["keep_scale"], lens=lens, t=case["t"], small=small,
                             bf16=(2 if w16 else False) if bf16 is None else bf16)
    except native.NativeError:
        _sync(dev)
        assert all(s is None or bool(torch.isnan(s.whole).all()) for s in out.values()), "a refused call wrote its outputs"
        raise
    _sync(dev)
    for n, s in out.items():
        assert s is None or s.intact(), "written beside " + n
    return {n: None if s is None else s.numpy() for n, s in out.items()}


def lstm_label(case):
    none = [n for n in ("gin", "bias", "c_prev") if case[n] is None]
    parts = ["B %d H %d widths %s weights %s" % (case["B"], case["H"], ",".join(
        ("(%d)" if x is None else "%d") % w for x, w in zip(case["xs"], case["widths"])), case["fmt"])]
    parts += ["no " + " ".join(none)] if none else []
    parts += ["keep"] if case["keep"] is not None else []
    parts += ["lens %s t %d" % (",".join(map(str, case["lens"])), case["t"])] if case["lens"] is not None else []
    return ", ".join(parts)


def check_lstm(case, out, label=""):
    """gates, c and h under the tolerance; rows past their length bit-exact +0; prints the FIGURE ratios."""
    worst = {}
    for n in ("gates", "c", "h"):
        if out[n] is None:
            continue
        assert np.isfinite(out[n]).all(), (label, n, "not finite")
        if case["lens"] is not None:
            assert not bits(out[n][case["t"] >= case["lens"]]).any(), (label, n, "rows past their length")
        worst[n] = fr.error(out[n], case["f64"][n]) / fr.allowed(case["f32"][n], case["f64"][n])
    print("FIGURE small_batch lstm %s(%s): error / allowed %s"
          % (label, lstm_label(case), " ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst
    return worst


def run_linear(case, dev, x_pad=4, x_lead=4, w_pad=4, w_lead=4):
    """native.linear_small on the case -> numpy Y.  x_pad = 1 and x_lead = 1 give the scalar staging path (ldx = K + 1, a base
    one float into its buffer)."""
    from tacotron2_amd import native
    X = Slab(dev, data=case["X"], pad=x_pad, lead=x_lead)
    W = Slab(dev, data=case["W"], pad=w_pad, lead=w_lead)
    bias = None if case["bias"] is None else Slab(dev, data=case["bias"][None], pad=3)
    keep = None if case["keep"] is None else Slab(dev, data=case["keep"], pad=3, dtype=torch.uint8, fill=1)
    Y = Slab(dev, case["B"], case["N"], pad=3)
    try:
        native.linear_small(X.view, W.view, Y.view, bias=None if bias is None else bias.view[0], act=case["act"],
                            keep=None if keep is None else keep.view, keep_scale=case["keep_scale"])
    except native.NativeError:
        _sync(dev)
        assert bool(torch.isnan(Y.whole).all()), "a refused call wrote its output"
        raise
    _sync(dev)
    assert Y.intact(), "written beside Y"
    return Y.numpy()


def check_linear(case, y, label=""):
    assert np.isfinite(y).all(), (label, "not finite")
    ratio = fr.error(y, case["f64"]) / fr.allowed(case["f32"], case["f64"])
    print("FIGURE small_batch linear %s(B %d N %d K %d act %d bias %d keep %d): error / allowed y %.3f"
          % (label, case["B"], case["N"], case["K"], case["act"], case["bias"] is not None, case["keep"] is not None, ratio))
    assert ratio <= 1.0, ratio
    return ratio


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def refusals():
    """(name, call) pairs: each ``call(dev)`` must raise NativeError before anything is launched; its outputs are checked to be
    untouched by the runners (a call that went through would return).  Cases without restatements: nothing is computed."""
    def lstm(B, H, widths, fmt="f32", **kw):
        K = sum(widths)
        case = dict(B=B, H=H, widths=tuple(widths), fmt=fmt, W=np.zeros((4 * H, K), F32), t=0, keep_scale=1.0,
                    xs=[np.zeros((B, w), F32) for w in widths], gin=None, bias=None, c_prev=None, keep=None, lens=None)
        return lambda dev: run_lstm(case, dev, **kw)

    def linear(B, N, K, **kw):
        case = dict(B=B, N=N, K=K, act=0, keep_scale=1.0, X=np.zeros((B, K), F32), W=np.zeros((N, K), F32), bias=None, keep=None)
        return lambda dev: run_linear(case, dev, **kw)

    def bf16_operands(dev):
        from tacotron2_amd import native
        x, W = torch.zeros(2, 16, dtype=torch.bfloat16, device=dev), torch.zeros(32, 16, dtype=torch.bfloat16, device=dev)
        c, h = Slab(dev, 2, 8), Slab(dev, 2, 8)
        try:
            native.lstm_step_fwd([x], [16], W, 8, 2, None, c.view, h.view, small=True, bf16=True)
        finally:
            _sync(dev)
            assert c.intact() and h.intact() and torch.isnan(c.view).all() and torch.isnan(h.view).all()

    return (("lstm B = 9", lstm(9, 8, (16,))),
            ("linear B = 9", linear(9, 16, 16)),
            ("lstm K % 4", lstm(2, 8, (8, 6, 10))),
            ("linear K % 4", linear(2, 16, 18, x_pad=2, w_pad=2)),
            ("lstm H % 4", lstm(2, 6, (16,))),
            ("bf16 weights K % 8", lstm(2, 8, (8, 4), "bf16")),
            ("bf16 operands in the matrix-vector form", bf16_operands),
            ("lstm weight base 4 bytes off", lstm(2, 8, (16,), w_lead=1)),
            ("lstm bf16 weight base 8 bytes off", lstm(2, 8, (16,), "bf16", w_lead=4)),
            ("linear weight base 4 bytes off", linear(2, 16, 16, w_lead=1)),
            ("lstm B = 8 K = 5120 beyond the LDS", lstm(8, 4, (2048, 1024, 2048))),
            ("lstm bf16 B = 8 K = 5120 beyond the LDS", lstm(8, 4, (2048, 1024, 2048), "bf16")))
