"""The host layer of the alignment, regulator and Transformer ops (tacotron2_amd/ragged.py and the argument helpers of native.py):
every refusal keeps its exception type and its text, and a good call hands the C entries the integers it always did.  The
expected strings and integers below were recorded on the commit before the layer was shared; they are literals, never computed
from the code under test.  Everything runs in validate-only mode on host tensors: the checks run, no kernel does."""
import ctypes

import pytest
import torch

from tacotron2_amd import alignment as al
from tacotron2_amd import native as nv
from tacotron2_amd import transformer as tr

I32, I64, U8 = torch.int32, torch.int64, torch.uint8
INF, NAN = float("inf"), float("nan")


def Z(*shape, **kw):
    return torch.zeros(*shape, **kw)


def meta(*shape, **kw):
    return torch.zeros(*shape, device="meta", **kw)


def ints(*v):
    return torch.tensor(v, dtype=I32)


def ws(n=1 << 16, dtype=U8):
    return torch.zeros(n, dtype=dtype)


def outcome(fn):
    """'Type: text' of what ``fn`` raises, or 'ok' with the ints it returns."""
    try:
        r = fn()
    except Exception as e:                                                  # noqa: BLE001 -- the type is what is recorded
        return "%s: %s" % (type(e).__name__, e)
    return "ok %r" % (r,) if isinstance(r, (int, tuple, str)) else "ok"


class Recorder:
    """A stand-in for ``native._lib``: passes every call on and keeps the name and the arguments of each ``t2amd_*`` launch or
    query, a pointer as ``*`` or ``NULL``; ``ptrs`` holds the pointers themselves."""
    QUIET = ("t2amd_last_error", "t2amd_set_validate_only")

    def __init__(self, lib):
        self.lib, self.calls, self.ptrs = lib, [], []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("t2amd_") or name in self.QUIET:
            return fn

        def call(*args):
            words = []
            for a in args:
                if a is None:
                    words.append("NULL")
                elif isinstance(a, ctypes.c_void_p):
                    words.append("*")
                    self.ptrs.append(a.value)
                elif isinstance(a, (int, float)):
                    words.append(repr(a))
                elif isinstance(a, ctypes._SimpleCData):
                    words.append(repr(a.value))
                else:
                    words.append("*")                                       # byref of a result cell
            self.calls.append("%s(%s)" % (name[6:], " ".join(words)))
            return fn(*args)
        return call


def recorded(fn):
    """The calls ``fn`` makes, then whatever string it returns."""
    rec = Recorder(nv.load())
    saved, nv._lib = nv._lib, rec
    try:
        note = fn(rec)
    finally:
        nv._lib = saved
    return rec.calls + ([note] if isinstance(note, str) else [])


@pytest.fixture
def dry(native_lib):
    nv.set_validate_only(True)
    yield
    nv.set_validate_only(False)


# ---- refusals: the public functions ------------------------------------------------------------------------------------------------
S, Q, X = Z(2, 5, 3), Z(2, 6, 2, 32), Z(2, 6, 32)
D23 = torch.ones(2, 3, dtype=I32)
W3 = Z(32, 32, 3)


def _path_refusals(name, f):
    return {
        name + " dtype": lambda: f(S.double()),
        name + " no tensor": lambda: f([[0.0]]),
        name + " rank": lambda: f(Z(5)),
        name + " empty": lambda: f(Z(2, 0, 3)),
        name + " count": lambda: f(S, [5], None),
        name + " n count": lambda: f(S, None, [3, 3, 3]),
        name + " frames high": lambda: f(S, [5, 6], [3, 3]),
        name + " tokens low": lambda: f(S, [5, 5], [3, 0]),
        name + " more tokens": lambda: f(Z(2, 3, 5)),
        name + " more tokens in one": lambda: f(S, [5, 2], [3, 3]),
        name + " frame limit": lambda: f(Z(1, 4097, 2)),
        name + " token limit": lambda: f(Z(1, 1025, 1025)),
        name + " host": None,
    }


REFUSALS = {}
for _n, _f in (("monotonic_align", al.monotonic_align), ("forward_sum", al.forward_sum), ("alignment_posterior", al.alignment_posterior),
               ("ForwardSumLoss", al.ForwardSumLoss())):
    REFUSALS.update({k: v for k, v in _path_refusals(_n, _f).items() if v is not None})
REFUSALS.update({
    "ForwardSumLoss reduction": lambda: al.ForwardSumLoss("median"),
    "attention_durations no tensor": lambda: al.attention_durations([[1.0]], [1], [1]),
    "alignment_metrics shapes": lambda: al.alignment_metrics(Z(2, 5, 3), Z(2, 4), None, None),
    "alignment_metrics path": lambda: al.alignment_metrics(Z(1, 5, 3), torch.full((1, 5), 3), None, None),
    "alignment_metrics lengths": lambda: al.alignment_metrics(Z(1, 5, 3), Z(1, 5), [4], None),
    "aligner_scores dtype q": lambda: al.aligner_scores(Z(2, 5, 4).half(), Z(2, 3, 4)),
    "aligner_scores dtype k": lambda: al.aligner_scores(Z(2, 5, 4), [[1.0]]),
    "aligner_scores dtype prior": lambda: al.aligner_scores(Z(2, 5, 4), Z(2, 3, 4), log_prior=Z(2, 5, 3).double()),
    "aligner_scores rank": lambda: al.aligner_scores(Z(5, 4), Z(2, 3, 4)),
    "aligner_scores empty": lambda: al.aligner_scores(Z(2, 0, 4), Z(2, 3, 4)),
    "aligner_scores batch": lambda: al.aligner_scores(Z(2, 5, 4), Z(3, 3, 4)),
    "aligner_scores channels": lambda: al.aligner_scores(Z(2, 5, 4), Z(2, 3, 5)),
    "aligner_scores channel limit": lambda: al.aligner_scores(Z(1, 2, 513), Z(1, 2, 513)),
    "aligner_scores prior shape": lambda: al.aligner_scores(Z(2, 5, 4), Z(2, 3, 4), log_prior=Z(2, 5, 4)),
    "aligner_scores frame limit": lambda: al.aligner_scores(Z(1, 4097, 4), Z(1, 3, 4)),
    "aligner_scores token limit": lambda: al.aligner_scores(Z(1, 5, 4), Z(1, 1025, 4)),
    "aligner_scores frames high": lambda: al.aligner_scores(Z(2, 5, 4), Z(2, 3, 4), [5, 6], [3, 3]),
    "aligner_scores tokens low": lambda: al.aligner_scores(Z(2, 5, 4), Z(2, 3, 4), [5, 5], [0, 3]),
    "aligner_scores count": lambda: al.aligner_scores(Z(2, 5, 4), Z(2, 3, 4), [5]),
    "aligner_scores keys elsewhere": lambda: al.aligner_scores(Z(2, 5, 4), meta(2, 3, 4)),
    "aligner_scores prior elsewhere": lambda: al.aligner_scores(Z(2, 5, 4), Z(2, 3, 4), log_prior=meta(2, 5, 3)),
    "beta_binomial none": lambda: al.beta_binomial_log_prior([], []),
    "beta_binomial count": lambda: al.beta_binomial_log_prior([5, 4], [3], device="cpu"),
    "beta_binomial range": lambda: al.beta_binomial_log_prior([5, 4], [3, 2], T=4, N=3, device="cpu"),
    "beta_binomial limit": lambda: al.beta_binomial_log_prior([4097], [3], device="cpu"),
    "AlignerScores prior lengths": lambda: al.AlignerScores(prior_scaling=1.0)(Z(2, 5, 4), Z(2, 3, 4), [5, 6]),
    "durations_to_path dtype": lambda: al.durations_to_path(Z(2, 3)),
    "durations_to_path no tensor": lambda: al.durations_to_path([1, 2]),
    "durations_to_path rank": lambda: al.durations_to_path(Z(2, 3, 4, dtype=I32), T=4),
    "durations_to_path empty": lambda: al.durations_to_path(Z(2, 0, dtype=I32), T=4),
    "durations_to_path token limit": lambda: al.durations_to_path(Z(1, 1025, dtype=I32), T=4),
    "durations_to_path lengths elsewhere": lambda: al.durations_to_path(D23, meta(2, dtype=I32), T=4),
    "durations_to_path device count": lambda: al.durations_to_path(meta(2, 3, dtype=I32), meta(3, dtype=I32), T=4),
    "durations_to_path device rank": lambda: al.durations_to_path(meta(2, 3, dtype=I32), meta(2, 1, dtype=I32), T=4),
    "durations_to_path count": lambda: al.durations_to_path(D23, [3], T=4),
    "durations_to_path tokens high": lambda: al.durations_to_path(D23, [4, 1], T=4),
    "durations_to_path tokens low": lambda: al.durations_to_path(D23, [3, -1], T=4),
    "length_regulate dtype": lambda: al.length_regulate(Z(2, 3, 4).double(), D23, T=4),
    "length_regulate rank": lambda: al.length_regulate(Z(2, 3, 4, 5), D23, T=4),
    "length_regulate empty": lambda: al.length_regulate(Z(2, 3, 0), D23, T=4),
    "length_regulate durations elsewhere": lambda: al.length_regulate(Z(2, 3, 4), meta(2, 3, dtype=I32), T=4),
    "length_regulate durations dtype": lambda: al.length_regulate(Z(2, 3, 4), Z(2, 3), T=4),
    "length_regulate durations shape": lambda: al.length_regulate(Z(2, 3, 4), torch.ones(2, 4, dtype=I32), T=4),
    "length_regulate flat durations": lambda: al.length_regulate(Z(2, 3, 4), torch.ones(3, dtype=I32), T=4),
    "length_regulate channel limit": lambda: al.length_regulate(Z(2, 3, 513), D23, T=4),
    "length_regulate tokens high": lambda: al.length_regulate(Z(2, 3, 4), D23, [3, 4], T=4),
    "token_average dtype": lambda: al.token_average(Z(2, 5).double(), D23),
    "token_average rank": lambda: al.token_average(Z(5), D23),
    "token_average empty": lambda: al.token_average(Z(2, 0), D23),
    "token_average frame limit": lambda: al.token_average(Z(1, 65537), D23[:1]),
    "token_average channel limit": lambda: al.token_average(Z(2, 5, 513), D23),
    "token_average durations elsewhere": lambda: al.token_average(Z(2, 5), meta(2, 3, dtype=I32)),
    "token_average batch": lambda: al.token_average(Z(3, 5), D23),
    "token_average weights dtype": lambda: al.token_average(Z(2, 5), D23, weights=Z(2, 5).double()),
    "token_average weights shape": lambda: al.token_average(Z(2, 5), D23, weights=Z(2, 4)),
    "token_average weights elsewhere": lambda: al.token_average(Z(2, 5), D23, weights=meta(2, 5)),
    "self_attention dtype q": lambda: tr.self_attention(Q.double(), Q, Q),
    "self_attention dtype k": lambda: tr.self_attention(Q, Q.half(), Q),
    "self_attention dtype v": lambda: tr.self_attention(Q, Q, [[0.0]]),
    "self_attention batch": lambda: tr.self_attention(Q, Q[:1], Q),
    "self_attention rank": lambda: tr.self_attention(Z(6, 32), Z(6, 32), Z(6, 32)),
    "self_attention empty": lambda: tr.self_attention(*(Z(2, 0, 2, 32),) * 3),
    "self_attention width": lambda: tr.self_attention(*(Z(1, 2, 1, 48),) * 3),
    "self_attention heads": lambda: tr.self_attention(*(Z(1, 2, 17, 32),) * 3),
    "self_attention frames": lambda: tr.self_attention(*(Z(1, 4097, 1, 32),) * 3),
    "self_attention batch heads": lambda: tr.self_attention(*(Z(4096, 1, 16, 32),) * 3),
    "self_attention k elsewhere": lambda: tr.self_attention(Q, meta(2, 6, 2, 32), Q),
    "self_attention lengths elsewhere": lambda: tr.self_attention(Q, Q, Q, meta(2, dtype=I32)),
    "self_attention device count": lambda: tr.self_attention(*(meta(2, 6, 2, 32),) * 3, meta(3, dtype=I32)),
    "self_attention device float": lambda: tr.self_attention(*(meta(2, 6, 2, 32),) * 3, meta(2)),
    "self_attention count": lambda: tr.self_attention(Q, Q, Q, [6]),
    "self_attention frames high": lambda: tr.self_attention(Q, Q, Q, [6, 7]),
    "self_attention frames low": lambda: tr.self_attention(Q, Q, Q, [-1, 3]),
    "MultiHeadSelfAttention heads": lambda: tr.MultiHeadSelfAttention(17, 64, 32),
    "MultiHeadSelfAttention width": lambda: tr.MultiHeadSelfAttention(2, 64, 40),
    "MultiHeadSelfAttention d_model": lambda: tr.MultiHeadSelfAttention(2, True, 32),
    "MultiHeadSelfAttention x": lambda: tr.MultiHeadSelfAttention(1, 32, 32)(Z(2, 5, 31)),
    "ragged_conv1d dtype": lambda: tr.ragged_conv1d(X.double(), W3),
    "ragged_conv1d rank": lambda: tr.ragged_conv1d(Z(6, 32), W3),
    "ragged_conv1d empty": lambda: tr.ragged_conv1d(Z(2, 0, 32), W3),
    "ragged_conv1d frames": lambda: tr.ragged_conv1d(Z(1, 4097, 32), W3),
    "ragged_conv1d batch": lambda: tr.ragged_conv1d(Z(65536, 1, 32), W3),
    "ragged_conv1d weight dtype": lambda: tr.ragged_conv1d(X, W3.double()),
    "ragged_conv1d weight shape": lambda: tr.ragged_conv1d(X, Z(32, 64, 3)),
    "ragged_conv1d even": lambda: tr.ragged_conv1d(X, Z(32, 32, 2)),
    "ragged_conv1d wide": lambda: tr.ragged_conv1d(X, Z(32, 32, 11)),
    "ragged_conv1d channels in": lambda: tr.ragged_conv1d(Z(2, 6, 48), Z(32, 48, 3)),
    "ragged_conv1d channels out": lambda: tr.ragged_conv1d(X, Z(4128, 32, 1)),
    "ragged_conv1d weight elsewhere": lambda: tr.ragged_conv1d(X, meta(32, 32, 3)),
    "ragged_conv1d bias dtype": lambda: tr.ragged_conv1d(X, W3, Z(32).double()),
    "ragged_conv1d bias shape": lambda: tr.ragged_conv1d(X, W3, Z(31)),
    "ragged_conv1d bias elsewhere": lambda: tr.ragged_conv1d(X, W3, meta(32)),
    "ragged_conv1d lengths elsewhere": lambda: tr.ragged_conv1d(X, W3, None, meta(2, dtype=I32)),
    "ragged_conv1d frames high": lambda: tr.ragged_conv1d(X, W3, None, [6, 7]),
    "ragged_conv1d count": lambda: tr.ragged_conv1d(X, W3, None, [6, 6, 6]),
    "add_layer_norm dtype": lambda: tr.add_layer_norm(X.half()),
    "add_layer_norm rank": lambda: tr.add_layer_norm(Z(6, 32)),
    "add_layer_norm narrow": lambda: tr.add_layer_norm(Z(2, 6, 28)),
    "add_layer_norm odd": lambda: tr.add_layer_norm(Z(2, 6, 34)),
    "add_layer_norm residual shape": lambda: tr.add_layer_norm(X, Z(2, 5, 32)),
    "add_layer_norm residual dtype": lambda: tr.add_layer_norm(X, X.double()),
    "add_layer_norm weight alone": lambda: tr.add_layer_norm(X, None, Z(32)),
    "add_layer_norm weight shape": lambda: tr.add_layer_norm(X, None, Z(31), Z(32)),
    "add_layer_norm bias elsewhere": lambda: tr.add_layer_norm(X, None, Z(32), meta(32)),
    "add_layer_norm frames low": lambda: tr.add_layer_norm(X, lengths=[-1, 2]),
    "PositionwiseConvFF kernel": lambda: tr.PositionwiseConvFF(32, 32, 4),
    "PositionwiseConvFF pair": lambda: tr.PositionwiseConvFF(32, 32, (3, True)),
    "PositionwiseConvFF d_inner": lambda: tr.PositionwiseConvFF(32, 48, 3),
    "PositionwiseConvFF x": lambda: tr.PositionwiseConvFF(32, 32, 3)(Z(2, 6, 31)),
    "PositionwiseConvFF lengths": lambda: tr.PositionwiseConvFF(32, 32, 3)(X, [6, 7]),
    "FFTBlock lengths": lambda: tr.FFTBlock(1, 32, 32, 32, 3)(X, [7, 6]),
    "FFTransformer n_layer": lambda: tr.FFTransformer(0, 1, 32, 32, 32, 3),
    "FFTransformer x": lambda: tr.FFTransformer(1, 1, 32, 32, 32, 3)(Z(2, 6)),
    "FFTransformer symbols": lambda: tr.FFTransformer(1, 1, 32, 32, 32, 3, n_embed=5)(X),
    "FFTransformer lengths": lambda: tr.FFTransformer(1, 1, 32, 32, 32, 3)(X, [6]),
    "FFTransformer lengths elsewhere": lambda: tr.FFTransformer(1, 1, 32, 32, 32, 3)(X, meta(2, dtype=I32)),
})
for _v in (True, 0, 0.0, -1.0, INF, NAN, "1", None):                       # the scalars: each op keeps its own idea of a number
    _k = " %r" % (_v,)
    REFUSALS.update({
        "aligner_scores temperature" + _k: lambda v=_v: al.aligner_scores(Z(1, 2, 4), Z(1, 2, 4), temperature=v) is None,
        "AlignerScores temperature" + _k: lambda v=_v: al.AlignerScores(temperature=v) is None,
        "AlignerScores prior_scaling" + _k: lambda v=_v: al.AlignerScores(prior_scaling=v) is None,
        "beta_binomial scaling" + _k: lambda v=_v: al.beta_binomial_log_prior([2], [2], v, device="cpu") is None,
        "LengthRegulator pace" + _k: lambda v=_v: al.LengthRegulator(pace=v) is None,
        "self_attention scale" + _k: lambda v=_v: tr.self_attention(Q, Q, Q, scale=v) is None,
        "add_layer_norm eps" + _k: lambda v=_v: tr.add_layer_norm(X, eps=v) is None,
    })
for _v in (True, -1, 65537, 1.5, "4"):
    _k = " %r" % (_v,)
    REFUSALS.update({
        "durations_to_path T" + _k: lambda v=_v: al.durations_to_path(D23, T=v) is None,
        "length_regulate T" + _k: lambda v=_v: al.length_regulate(Z(2, 3, 4), D23, T=v) is None,
        "LengthRegulator max_len" + _k: lambda v=_v: al.LengthRegulator(max_len=v) is None,
    })
REFUSALS["beta_binomial scaling 10000000.0"] = lambda: al.beta_binomial_log_prior([2], [2], 1e7, device="cpu") is None
REFUSALS["AlignerScores prior_scaling 10000000.0"] = lambda: al.AlignerScores(prior_scaling=1e7) is None

# outside validate-only mode a host tensor is refused: "no CPU path", in each module's own words
HOST_REFUSALS = {
    "monotonic_align": lambda: al.monotonic_align(Z(1, 2, 2)),
    "forward_sum": lambda: al.forward_sum(Z(1, 2, 2)),
    "aligner_scores": lambda: al.aligner_scores(Z(1, 2, 4), Z(1, 2, 4)),
    "beta_binomial_log_prior": lambda: al.beta_binomial_log_prior([2], [2], device="cpu"),
    "durations_to_path": lambda: al.durations_to_path(D23, T=4),
    "length_regulate": lambda: al.length_regulate(Z(2, 3, 4), D23, T=4),
    "token_average": lambda: al.token_average(Z(2, 5), D23),
    "self_attention": lambda: tr.self_attention(Q, Q, Q),
    "ragged_conv1d": lambda: tr.ragged_conv1d(X, W3),
    "add_layer_norm": lambda: tr.add_layer_norm(X),
    "MultiHeadSelfAttention": lambda: tr.MultiHeadSelfAttention(1, 32, 32)(X),
}

# ---- refusals and queries: the native wrappers -----------------------------------------------------------------------------------------
L2, F2 = ints(5, 4), Z(2)
NATIVE = {
    "align_limits": nv.align_limits,
    "regulate_limits": nv.regulate_limits,
    "self_attn_limits": nv.self_attn_limits,
    "fft_block_limits": nv.fft_block_limits,
    "align_workspace": lambda: nv.align_workspace(2, 5, 3),
    "align_workspace frames": lambda: nv.align_workspace(2, 4097, 3),
    "align_workspace tokens": lambda: nv.align_workspace(2, 2000, 1025),
    "align_workspace empty": lambda: nv.align_workspace(0, 5, 3),
    "forward_sum_workspace": lambda: (nv.forward_sum_workspace(2, 5, 3, True), nv.forward_sum_workspace(2, 5, 3, False)),
    "forward_sum_workspace frames": lambda: nv.forward_sum_workspace(2, 4097, 3),
    "aligner_workspace": lambda: tuple(nv.aligner_workspace(2, 5, 3, 4, w) for w in (0, 1, 2)),
    "aligner_workspace which": lambda: nv.aligner_workspace(2, 5, 3, 4, 3),
    "aligner_workspace channels": lambda: nv.aligner_workspace(2, 5, 3, 513),
    "self_attn_workspace": lambda: tuple(nv.self_attn_workspace(3, 10, 2, 32, w) for w in (0, 1, 2)),
    "self_attn_workspace width": lambda: nv.self_attn_workspace(3, 10, 2, 48),
    "self_attn_workspace heads": lambda: nv.self_attn_workspace(3, 10, 17, 32),
    "fft_block_workspace": lambda: tuple(nv.fft_block_workspace(2, 6, 32, 64, 3, w) for w in (0, 1, 2)),
    "fft_block_workspace kernel": lambda: nv.fft_block_workspace(2, 6, 32, 64, 4, 1),
    "fft_block_workspace channels": lambda: nv.fft_block_workspace(2, 6, 4128, 64, 3, 1),
    "monotonic_align rank": lambda: nv.monotonic_align(Z(5, 3), L2, L2, Z(2, 3, dtype=I32), F2, None, ws()),
    "monotonic_align stride": lambda: nv.monotonic_align(Z(2, 3, 5).transpose(1, 2), L2, L2, Z(2, 3, dtype=I32), F2, None, ws()),
    "monotonic_align durations": lambda: nv.monotonic_align(S, L2, L2, Z(2, 4, dtype=I32), F2, None, ws()),
    "monotonic_align path": lambda: nv.monotonic_align(S, L2, L2, Z(2, 3, dtype=I32), F2, Z(2, 4, dtype=I32), ws()),
    "monotonic_align workspace dtype": lambda: nv.monotonic_align(S, L2, ints(3, 2), Z(2, 3, dtype=I32), F2, None, ws(dtype=torch.float32)),
    "monotonic_align workspace stride": lambda: nv.monotonic_align(S, L2, ints(3, 2), Z(2, 3, dtype=I32), F2, None, ws()[::2]),
    "monotonic_align workspace small": lambda: nv.monotonic_align(S, L2, ints(3, 2), Z(2, 3, dtype=I32), F2, None, ws(8)),
    "monotonic_align lengths dtype": lambda: nv.monotonic_align(S, L2.long(), ints(3, 2), Z(2, 3, dtype=I32), F2, None, ws()),
    "monotonic_align lengths count": lambda: nv.monotonic_align(S, L2, ints(3), Z(2, 3, dtype=I32), F2, None, ws()),
    "monotonic_align expanded": lambda: nv.monotonic_align(Z(1, 5, 3).expand(2, 5, 3), L2, ints(3, 2), Z(2, 3, dtype=I32), F2, None, ws()),
    "forward_sum rank": lambda: nv.forward_sum(Z(5, 3), L2, L2, F2, ws()),
    "forward_sum log_z": lambda: nv.forward_sum(S, L2, ints(3, 2), Z(3), ws()),
    "forward_sum workspace": lambda: nv.forward_sum(S, L2, ints(3, 2), F2, ws(dtype=torch.int8)),
    "forward_sum lengths": lambda: nv.forward_sum(S, L2[::1].float(), ints(3, 2), F2, ws()),
    "forward_sum_backward grad shape": lambda: nv.forward_sum_backward(S, L2, ints(3, 2), F2, None, Z(2, 5, 4), None, ws()),
    "forward_sum_backward grad stride": lambda: nv.forward_sum_backward(S, L2, ints(3, 2), F2, None, Z(2, 3, 5).transpose(1, 2), None, ws()),
    "forward_sum_backward soft": lambda: nv.forward_sum_backward(S, L2, ints(3, 2), F2, None, Z(2, 5, 3), Z(2, 4), ws()),
    "forward_sum_backward workspace": lambda: nv.forward_sum_backward(S, L2, ints(3, 2), F2, None, Z(2, 5, 3), None, ws()[::2]),
    "aligner_scores operands": lambda: nv.aligner_scores(Z(2, 5, 4), Z(3, 3, 4), L2, ints(3, 2), 1.0, None, S, ws()),
    "aligner_scores shape": lambda: nv.aligner_scores(Z(2, 5, 4), Z(2, 3, 4), L2, ints(3, 2), 1.0, None, Z(2, 5, 4), ws()),
    "aligner_scores prior stride": lambda: nv.aligner_scores(Z(2, 5, 4), Z(2, 3, 4), L2, ints(3, 2), 1.0, Z(2, 3, 5).transpose(1, 2), S, ws()),
    "aligner_scores workspace": lambda: nv.aligner_scores(Z(2, 5, 4), Z(2, 3, 4), L2, ints(3, 2), 1.0, None, S, ws(dtype=I32)),
    "aligner_scores q stride": lambda: nv.aligner_scores(Z(2, 4, 5).transpose(1, 2), Z(2, 3, 4), L2, ints(3, 2), 1.0, None, S, ws()),
    "aligner_scores tau": lambda: nv.aligner_scores(Z(2, 5, 4), Z(2, 3, 4), L2, ints(3, 2), 0.0, None, S, ws()),
    "aligner_scores_backward shapes": lambda: nv.aligner_scores_backward(Z(2, 5, 4), Z(2, 3, 4), L2, ints(3, 2), 1.0, S, Z(2, 5, 4), Z(2, 3, 5),
                                                                        None, ws(), ws()),
    "aligner_scores_backward kept": lambda: nv.aligner_scores_backward(Z(2, 5, 4), Z(2, 3, 4), L2, ints(3, 2), 1.0, S, Z(2, 5, 4), Z(2, 3, 4),
                                                                      None, ws(dtype=I32), ws()),
    "beta_binomial_log_prior rank": lambda: nv.beta_binomial_log_prior(L2, ints(3, 2), 1.0, Z(5, 3)),
    "beta_binomial_log_prior stride": lambda: nv.beta_binomial_log_prior(L2, ints(3, 2), 1.0, Z(2, 3, 5).transpose(1, 2)),
    "durations_to_path dtype": lambda: nv.durations_to_path(Z(2, 3), None, 4, None, Z(2, dtype=I32)),
    "durations_to_path stride": lambda: nv.durations_to_path(Z(3, 2, dtype=I32).t(), None, 4, None, Z(2, dtype=I32)),
    "durations_to_path totals": lambda: nv.durations_to_path(D23, None, 4, None, Z(2, dtype=I32), None, Z(2, dtype=I32)),
    "durations_to_path path": lambda: nv.durations_to_path(D23, None, 4, Z(2, 5, dtype=I32), Z(2, dtype=I32)),
    "durations_to_path ends": lambda: nv.durations_to_path(D23, None, 4, None, Z(2, dtype=I32), Z(2, 3, dtype=I64)),
    "durations_to_path t_lengths": lambda: nv.durations_to_path(D23, None, 4, None, Z(4, dtype=I32)[::2]),
    "durations_to_path frames": lambda: nv.durations_to_path(D23, None, 65537, None, Z(2, dtype=I32)),
    "length_regulate stride": lambda: nv.length_regulate(Z(2, 4, 3).transpose(1, 2), Z(2, 5, dtype=I32), Z(2, 5, 4)),
    "length_regulate y": lambda: nv.length_regulate(Z(2, 3, 4), Z(2, 5, dtype=I32), Z(2, 5, 3)),
    "length_regulate path": lambda: nv.length_regulate(Z(2, 3, 4), Z(2, 5, dtype=I64), Z(2, 5, 4)),
    "length_regulate channels": lambda: nv.length_regulate(Z(2, 3, 513), Z(2, 5, dtype=I32), Z(2, 5, 513)),
    "length_regulate_backward rank": lambda: nv.length_regulate_backward(Z(5, 4), Z(2, 3, dtype=I32), Z(2, 3, 4)),
    "length_regulate_backward dx": lambda: nv.length_regulate_backward(Z(2, 5, 4), Z(2, 3, dtype=I32), Z(3, 3, 4)),
    "length_regulate_backward ends": lambda: nv.length_regulate_backward(Z(2, 5, 4), Z(2, 4, dtype=I32), Z(2, 3, 4)),
    "token_average values": lambda: nv.token_average(Z(2, 4, 5).transpose(1, 2), None, Z(2, 3, dtype=I32), Z(2, 3, 4), Z(2, 3)),
    "token_average mean": lambda: nv.token_average(Z(2, 5, 4), None, Z(2, 3, dtype=I32), Z(2, 3, 4), Z(2, 4)),
    "token_average weights": lambda: nv.token_average(Z(2, 5, 4), Z(5, 2).t(), Z(2, 3, dtype=I32), Z(2, 3, 4), Z(2, 3)),
    "token_average_backward shapes": lambda: nv.token_average_backward(Z(2, 3, 4), Z(2, 4), None, Z(2, 5, dtype=I32), Z(2, 5, 4)),
    "token_average_backward path": lambda: nv.token_average_backward(Z(2, 3, 4), Z(2, 3), None, Z(2, 6, dtype=I32), Z(2, 5, 4)),
    "self_attn stride": lambda: nv.self_attn(Z(2, 6, 32, 2).transpose(2, 3), Q, Q, None, 1.0, Z(2, 6, 2, 32)),
    "self_attn k shape": lambda: nv.self_attn(Q, Z(2, 5, 2, 32), Q, None, 1.0, Z(2, 6, 2, 32)),
    "self_attn rank": lambda: nv.self_attn(X, X, X, None, 1.0, X),
    "self_attn lse": lambda: nv.self_attn(Q, Q, Q, None, 1.0, Z(2, 6, 2, 32), Z(2, 6, 2).transpose(1, 2)),
    "self_attn o stride": lambda: nv.self_attn(Q, Q, Q, None, 1.0, Z(2, 2, 6, 32).transpose(1, 2)),
    "self_attn width": lambda: nv.self_attn(*(Z(1, 2, 1, 48),) * 3, None, 1.0, Z(1, 2, 1, 48)),
    "self_attn unaligned": lambda: nv.self_attn(Z(2 * 6 * 2 * 32 + 1)[1:].view(2, 6, 2, 32), Q, Q, None, 1.0, Z(2, 6, 2, 32)),
    "self_attn odd stride": lambda: nv.self_attn(Z(2, 6, 2, 33)[..., :32], Q, Q, None, 1.0, Z(2, 6, 2, 32)),
    "self_attn scale": lambda: nv.self_attn(Q, Q, Q, None, 0.0, Z(2, 6, 2, 32)),
    "self_attn lengths": lambda: nv.self_attn(Q, Q, Q, ints(6, 6, 6), 1.0, Z(2, 6, 2, 32)),
    "self_attn_delta o": lambda: nv.self_attn_delta(Q, Z(2, 5, 2, 32), None, Z(2, 2, 6)),
    "self_attn_delta delta": lambda: nv.self_attn_delta(Q, Z(2, 6, 2, 32), None, Z(2, 6, 2)),
    "self_attn_backward workspace": lambda: nv.self_attn_backward(Q, Q, Q, Z(2, 6, 2, 32), Z(2, 2, 6), Z(2, 6, 2, 32), None, 1.0,
                                                                 Z(2, 6, 2, 32), Z(2, 6, 2, 32), Z(2, 6, 2, 32), ws(dtype=I32)),
    "self_attn_backward small": lambda: nv.self_attn_backward(Q, Q, Q, Z(2, 6, 2, 32), Z(2, 2, 6), Z(2, 6, 2, 32), None, 1.0,
                                                             Z(2, 6, 2, 32), Z(2, 6, 2, 32), Z(2, 6, 2, 32), ws(16)),
    "self_attn_backward dq": lambda: nv.self_attn_backward(Q, Q, Q, Z(2, 6, 2, 32), Z(2, 2, 6), Z(2, 6, 2, 32), None, 1.0,
                                                          Z(2, 2, 6, 32).transpose(1, 2), Z(2, 6, 2, 32), Z(2, 6, 2, 32), ws()),
    "ffb_conv rank": lambda: nv.ffb_conv(Z(6, 32), Z(32, 96), None, None, None, 3, False, Z(2, 6, 32)),
    "ffb_conv stride": lambda: nv.ffb_conv(Z(2, 32, 6).transpose(1, 2), Z(32, 96), None, None, None, 3, False, Z(2, 6, 32)),
    "ffb_conv image": lambda: nv.ffb_conv(X, Z(32, 95), None, None, None, 3, False, Z(2, 6, 32)),
    "ffb_conv bias": lambda: nv.ffb_conv(X, Z(32, 96), Z(64)[::2], None, None, 3, False, Z(2, 6, 32)),
    "ffb_conv y": lambda: nv.ffb_conv(X, Z(32, 96), None, None, None, 3, False, Z(2, 32, 6).transpose(1, 2)),
    "ffb_conv y rank": lambda: nv.ffb_conv(X, Z(32, 96), None, None, None, 3, False, Z(6, 32)),
    "ffb_conv even": lambda: nv.ffb_conv(X, Z(32, 64), None, None, None, 2, False, Z(2, 6, 32)),
    "ffb_conv odd stride": lambda: nv.ffb_conv(Z(2, 6, 33)[..., :32], Z(32, 96), None, None, None, 3, False, Z(2, 6, 32)),
    "ffb_conv_dw g": lambda: nv.ffb_conv_dw(Z(2, 5, 32), X, None, 3, Z(32, 32, 3), ws()),
    "ffb_conv_dw dw": lambda: nv.ffb_conv_dw(Z(2, 6, 32), X, None, 3, Z(32, 3, 32), ws()),
    "ffb_conv_dw workspace": lambda: nv.ffb_conv_dw(Z(2, 6, 32), X, None, 3, Z(32, 32, 3), ws(dtype=I32)),
    "ffb_add_ln rank": lambda: nv.ffb_add_ln(Z(6, 32), None, None, None, None, 1e-5, Z(6, 32)),
    "ffb_add_ln residual": lambda: nv.ffb_add_ln(X, Z(2, 5, 32), None, None, None, 1e-5, Z(2, 6, 32)),
    "ffb_add_ln mean": lambda: nv.ffb_add_ln(X, None, Z(32), Z(32), None, 1e-5, Z(2, 6, 32), Z(2, 6, 32), Z(2, 6, 1), Z(2, 6)),
    "ffb_add_ln eps": lambda: nv.ffb_add_ln(X, None, Z(32), Z(32), None, 0.0, Z(2, 6, 32)),
    "ffb_add_ln_backward rank": lambda: nv.ffb_add_ln_backward(X, Z(6, 32), Z(2, 6), Z(2, 6), Z(32), None, Z(2, 6, 32)),
    "ffb_add_ln_backward g": lambda: nv.ffb_add_ln_backward(Z(2, 32, 6).transpose(1, 2), X, Z(2, 6), Z(2, 6), Z(32), None, Z(2, 6, 32)),
    "ffb_colsum rank": lambda: nv.ffb_colsum(Z(6, 32), None, None, None, None, Z(32), None, ws()),
    "ffb_colsum dbias": lambda: nv.ffb_colsum(X, None, None, None, None, Z(31), None, ws()),
    "ffb_colsum workspace": lambda: nv.ffb_colsum(X, None, None, None, None, Z(32), None, ws()[::2]),
    "ffb_relu_mask rank": lambda: nv.ffb_relu_mask(Z(6, 32), Z(6, 32), None, Z(6, 32)),
    "ffb_relu_mask y": lambda: nv.ffb_relu_mask(X, Z(2, 6, 31), None, Z(2, 6, 32)),
    "dtw slab": lambda: nv.dtw(Z(2, 5, 4), Z(2, 6, 4), None, None, Z(2), Z(2, dtype=I32), Z(2, 8, 8)),
    "dtw slab batch": lambda: nv.dtw(Z(2, 5, 4), Z(2, 6, 4), None, None, Z(2), Z(2, dtype=I32), Z(3, 8, 8, dtype=U8)),
    "dtw lengths": lambda: nv.dtw(Z(2, 5, 4), Z(2, 6, 4), ints(5, 5, 5), None, Z(2), Z(2, dtype=I32)),
    "dtw_backtrack slab": lambda: nv.dtw_backtrack(Z(2, 8, 16, dtype=U8)[:, :, ::2], None, None, Z(2, dtype=I32), 5, 6, Z(2, 11, 2, dtype=I32)),
    "mel_cepstrum stride": lambda: nv.mel_cepstrum(Z(2, 5, 8).transpose(1, 2), None, Z(3, 8), Z(2, 5, 3)),
    "mel_cepstrum lengths": lambda: nv.mel_cepstrum(Z(2, 8, 5), L2.long(), Z(3, 8), Z(2, 5, 3)),
    "yin lengths": lambda: nv.yin(Z(2, 4096), ints(5), 1024, 256, 20, 400, 22050.0, 0.1, Z(2, 17), Z(2, 17, dtype=U8), Z(2, 17)),
}


# ---- good calls: what reaches C --------------------------------------------------------------------------------------------------------
def _grad(t):
    return t.clone().requires_grad_(True)


def _packed(rec):
    """The q | k | v chunks of one packed projection are read where they lie."""
    B, T, H, D = 2, 6, 2, 32
    q, k, v = (c.view(B, T, H, D) for c in Z(B, T, 3 * H * D).chunk(3, dim=2))
    tr.self_attention(q, k, v, [6, 4])
    return "read in place: %r" % ([p in rec.ptrs for p in (q.data_ptr(), k.data_ptr(), v.data_ptr())],)


def _unaligned(rec):
    """A tensor whose storage offset is off 16 bytes is copied."""
    q = Z(2 * 6 * 2 * 32 + 1)[1:].view(2, 6, 2, 32)
    assert q.data_ptr() % 16 == 4
    tr.self_attention(q, Q, Q)
    x = Z(2 * 6 * 32 + 3)[3:].view(2, 6, 32)
    tr.ragged_conv1d(x, W3)
    tr.add_layer_norm(x)
    return "copied: %r; every pointer on 16 bytes: %r" % ([p not in rec.ptrs for p in (q.data_ptr(), x.data_ptr())],
                                                         all(p % 16 == 0 for p in rec.ptrs))


def _ffn(rec):
    torch.manual_seed(0)
    m = tr.FFTransformer(1, 2, 64, 32, 96, (3, 1))
    out, _ = m(_grad(Z(2, 6, 64)), [6, 3])
    out.sum().backward()


CALLS = {
    "align ones": lambda rec: al.monotonic_align(Z(1, 1, 1), return_path=True),
    "align ragged": lambda rec: al.monotonic_align(S, [5, 4], [3, 2]),
    "align shorter": lambda rec: al.monotonic_align(Z(2, 8, 6), [5, 4], [3, 2], return_path=True),
    "align slice": lambda rec: al.monotonic_align(Z(2, 8, 6)[:, :5, :3]),
    "align transposed": lambda rec: al.monotonic_align(Z(2, 3, 5).transpose(1, 2)),
    "align one utterance": lambda rec: al.monotonic_align(Z(9, 6)[:5, :3]),
    "forward_sum backward": lambda rec: al.forward_sum(_grad(Z(2, 8, 6)), [5, 4], [3, 2]).sum().backward(),
    "forward_sum one frame": lambda rec: al.forward_sum(_grad(Z(3, 1, 1))).sum().backward(),
    "alignment_posterior": lambda rec: al.alignment_posterior(Z(2, 3, 5).transpose(1, 2), [5, 4], [3, 2]),
    "ForwardSumLoss": lambda rec: al.ForwardSumLoss(per_frame=True)(_grad(S), [5, 4], [3, 2]).backward(),
    "aligner expanded": lambda rec: al.aligner_scores(_grad(Z(2, 5, 4)), _grad(Z(2, 3, 4)), [5, 4], [3, 2], 0.5,
                                                      _grad(Z(1, 5, 3)).expand(2, 5, 3)).sum().backward(),
    "aligner ones": lambda rec: al.aligner_scores(_grad(Z(1, 4)), Z(1, 4)).sum().backward(),
    "aligner more tokens": lambda rec: al.aligner_scores(Z(2, 3, 40), Z(2, 7, 40), log_prior=Z(2, 7, 3).transpose(1, 2)),
    "AlignerScores prior": lambda rec: al.AlignerScores(0.001, 0.5)(Z(2, 5, 4), Z(2, 3, 4), [5, 4], [3, 2]),
    "durations_to_path": lambda rec: al.durations_to_path(Z(3, 4, dtype=I64).t(), [3, 0, 2, 1], T=7),
    "durations_to_path one": lambda rec: al.durations_to_path(torch.ones(1, dtype=I32), T=0),
    "length_regulate": lambda rec: al.length_regulate(_grad(Z(2, 4, 3)).transpose(1, 2), D23, ints(3, 2), T=7)[0].sum().backward(),
    "length_regulate slice": lambda rec: al.length_regulate(Z(2, 8, 6)[:, :3, :4], Z(2, 5, dtype=I32)[:, :3], T=1),
    "length_regulate no frames": lambda rec: al.length_regulate(_grad(Z(3, 4)), torch.ones(3, dtype=I32), T=0)[0].sum().backward(),
    "LengthRegulator": lambda rec: al.LengthRegulator(2.0, max_len=9)(Z(1, 1, 1), torch.full((1, 1), 3.0)),
    "token_average": lambda rec: al.token_average(_grad(Z(2, 5)), D23, [3, 2], Z(5, 2).t()).sum().backward(),
    "token_average channels": lambda rec: al.token_average(_grad(Z(2, 4, 5)).transpose(1, 2), D23, None, Z(2, 8)[:, :5]).sum().backward(),
    "self_attention backward": lambda rec: tr.self_attention(_grad(Q), Q, Q, [6, 0], 0.5).sum().backward(),
    "self_attention ones": lambda rec: tr.self_attention(*(Z(1, 1, 32),) * 3),
    "self_attention transposed": lambda rec: tr.self_attention(Z(2, 2, 6, 64).transpose(1, 2), Q.repeat(1, 1, 1, 2), Z(2, 6, 2, 128)[..., :64]),
    "self_attention packed": _packed,
    "unaligned": _unaligned,
    "ragged_conv1d backward": lambda rec: tr.ragged_conv1d(_grad(X), _grad(Z(64, 32, 5)), _grad(Z(64)), [6, 2], relu=True).sum().backward(),
    "ragged_conv1d slice": lambda rec: tr.ragged_conv1d(Z(2, 8, 64)[:, :6, 32:], W3),
    "ragged_conv1d transposed": lambda rec: tr.ragged_conv1d(Z(1, 32, 1).transpose(1, 2), Z(32, 32, 1)),
    "add_layer_norm backward": lambda rec: tr.add_layer_norm(_grad(X), _grad(X), _grad(Z(32)), _grad(Z(32)), [6, 5], 1e-3).sum().backward(),
    "add_layer_norm plain": lambda rec: tr.add_layer_norm(_grad(Z(2, 32, 6)).transpose(1, 2), None).sum().backward(),
    "FFTransformer": _ffn,
}

# ---- what the commit before the shared layer answered ------------------------------------------------------------------------------
_AUDIO = "NativeError: tacotron2_amd.audio: move the module to the MI355X first (.cuda()); there is no CPU path"
HOST_REFUSED = {k: _AUDIO for k in ("aligner_scores", "beta_binomial_log_prior", "durations_to_path", "forward_sum", "length_regulate",
                                    "monotonic_align", "token_average")}
HOST_REFUSED.update({
    "MultiHeadSelfAttention": "NativeError: self_attention: q, k and v are on cpu; move them to the MI355X first, there is no CPU path",
    "self_attention": "NativeError: self_attention: q, k and v are on cpu; move them to the MI355X first, there is no CPU path",
    "add_layer_norm": "NativeError: add_layer_norm: x is on cpu; move it to the MI355X first, there is no CPU path",
    "ragged_conv1d": "NativeError: ragged_conv1d: x is on cpu; move it to the MI355X first, there is no CPU path",
})

REFUSED = {}
for _n, _w in (("monotonic_align", "monotonic_align"), ("forward_sum", "forward_sum"), ("alignment_posterior", "forward_sum"),
               ("ForwardSumLoss", "forward_sum")):                          # the forward-sum family refuses in forward_sum's name
    REFUSED.update({_n + " " + k: v % _w for k, v in {
        "count": "ValueError: %s: t_1 lengths for a batch of 2",
        "dtype": "TypeError: %s: expected a float32 tensor, got torch.float64",
        "empty": "ValueError: %s: expected (B, T, N) or (T, N) scores, got shape (2, 0, 3)",
        "frame limit": "ValueError: %s: utterance 0: 4097 frames and 2 tokens exceed the limits of 4096 frames and 1024 tokens",
        "frames high": "ValueError: %s: utterance 1: 6 frames and 3 tokens do not lie in [1, 5] and [1, 3]",
        "more tokens": "ValueError: %s: utterance 0 has 5 tokens and only 3 frames; a monotonic path needs 1 <= N <= T",
        "more tokens in one": "ValueError: %s: utterance 1 has 3 tokens and only 2 frames; a monotonic path needs 1 <= N <= T",
        "n count": "ValueError: %s: n_3 lengths for a batch of 2",
        "no tensor": "TypeError: %s: expected a float32 tensor, got list",
        "rank": "ValueError: %s: expected (B, T, N) or (T, N) scores, got shape (5,)",
        "token limit": "ValueError: %s: utterance 0: 1025 frames and 1025 tokens exceed the limits of 4096 frames and 1024 tokens",
        "tokens low": "ValueError: %s: utterance 1: 5 frames and 0 tokens do not lie in [1, 5] and [1, 3]",
    }.items()})
for _n, _t, _ok in (("AlignerScores prior_scaling", "AlignerScores: prior_scaling must be None or lie in (0, 1e6]", (None, True)),
                    ("AlignerScores temperature", "AlignerScores: the temperature must be a positive number", (True,)),
                    ("LengthRegulator pace", "LengthRegulator: the pace must be a positive number", (True,)),
                    ("add_layer_norm eps", "add_layer_norm: eps must be a positive number", ()),
                    ("aligner_scores temperature", "aligner_scores: the temperature must be a positive number", (True,)),
                    ("beta_binomial scaling", "beta_binomial_log_prior: the scaling must lie in (0, 1e6]", (True,)),
                    ("self_attention scale", "self_attention: the scale must be a positive number", (None,))):
    for _v in (True, 0, 0.0, -1.0, INF, NAN, "1", None) + ((1e7,) if "scaling" in _n else ()):
        REFUSED["%s %r" % (_n, _v)] = "ok False" if any(_v is o for o in _ok) else "ValueError: %s, got %r" % (_t, _v)
for _n in ("LengthRegulator: max_len", "durations_to_path: T", "length_regulate: T"):
    for _v in (True, -1, 65537, 1.5, "4"):
        REFUSED["%s %r" % (_n.replace(":", ""), _v)] = "ValueError: %s must be None or an int in [0, 65536], got %r" % (_n, _v)
_QK = "ValueError: aligner_scores: expected queries (B, T, C) or (T, C) and keys (B, N, C) or (N, C), got shapes %s and %s"
_QKV = "ValueError: self_attention: expected q, k and v of one shape (B, T, H, D) or (T, H, D), got %s, %s and %s"
REFUSED.update({
    "AlignerScores prior lengths": "ValueError: aligner_scores: utterance 1: 6 frames and 3 tokens do not lie in [1, 5] and [1, 3]",
    "FFTBlock lengths": "ValueError: FFTBlock: utterance 0: 7 frames do not lie in [0, 6]",
    "FFTransformer lengths": "ValueError: FFTransformer: 1 lengths for a batch of 2",
    "FFTransformer lengths elsewhere": "ValueError: FFTransformer: x is on cpu and lengths on meta",
    "FFTransformer n_layer": "ValueError: FFTransformer: n_layer must be a positive int, got 0",
    "FFTransformer symbols": "ValueError: FFTransformer: expected integer symbols (B, T), got (2, 6, 32)",
    "FFTransformer x": "ValueError: FFTransformer: expected x (B, T, 32), got (2, 6)",
    "ForwardSumLoss reduction": "ValueError: ForwardSumLoss: reduction must be 'mean', 'sum' or 'none', got 'median'",
    "MultiHeadSelfAttention d_model": "ValueError: MultiHeadSelfAttention: d_model must be a positive int, got True",
    "MultiHeadSelfAttention heads": "ValueError: MultiHeadSelfAttention: 17 heads exceed the limit of 16",
    "MultiHeadSelfAttention width": "ValueError: MultiHeadSelfAttention: a head width of 40 is not one of 32, 64, 96, 128",
    "MultiHeadSelfAttention x": "ValueError: MultiHeadSelfAttention: expected x (B, T, 32), got (2, 5, 31)",
    "PositionwiseConvFF d_inner": "ValueError: PositionwiseConvFF: d_inner must be a multiple of 32, at most 4096, got 48",
    "PositionwiseConvFF kernel": "ValueError: PositionwiseConvFF: kernel_size must be an odd int up to 9 or a pair of them, got 4",
    "PositionwiseConvFF lengths": "ValueError: PositionwiseConvFF: utterance 1: 7 frames do not lie in [0, 6]",
    "PositionwiseConvFF pair": "ValueError: PositionwiseConvFF: kernel_size must be an odd int up to 9 or a pair of them, got (3, True)",
    "PositionwiseConvFF x": "ValueError: PositionwiseConvFF: expected x (B, T, 32), got (2, 6, 31)",
    "add_layer_norm bias elsewhere": "ValueError: add_layer_norm: x is on cpu and bias on meta",
    "add_layer_norm dtype": "TypeError: add_layer_norm: expected float32 x, got torch.float16",
    "add_layer_norm frames low": "ValueError: add_layer_norm: utterance 0: -1 frames do not lie in [0, 6]",
    "add_layer_norm narrow": "ValueError: add_layer_norm: 28 channels are not a multiple of 4 from 32 to 4096",
    "add_layer_norm odd": "ValueError: add_layer_norm: 34 channels are not a multiple of 4 from 32 to 4096",
    "add_layer_norm rank": "ValueError: add_layer_norm: expected x (B, T, C), got (6, 32)",
    "add_layer_norm residual dtype": "TypeError: add_layer_norm: expected float32 residual, got torch.float64",
    "add_layer_norm residual shape": "ValueError: add_layer_norm: expected residual (2, 6, 32), got (2, 5, 32)",
    "add_layer_norm weight alone": "ValueError: add_layer_norm: weight and bias are given together or not at all",
    "add_layer_norm weight shape": "ValueError: add_layer_norm: expected weight (32,), got (31,)",
    "aligner_scores batch": _QK % ("(2, 5, 4)", "(3, 3, 4)"),
    "aligner_scores channel limit": "ValueError: aligner_scores: 513 channels exceed the limit of 512",
    "aligner_scores channels": _QK % ("(2, 5, 4)", "(2, 3, 5)"),
    "aligner_scores count": "ValueError: aligner_scores: t_1 lengths for a batch of 2",
    "aligner_scores dtype k": "TypeError: aligner_scores: expected float32 keys, got list",
    "aligner_scores dtype prior": "TypeError: aligner_scores: expected float32 log_prior, got torch.float64",
    "aligner_scores dtype q": "TypeError: aligner_scores: expected float32 queries, got torch.float16",
    "aligner_scores empty": _QK % ("(2, 0, 4)", "(2, 3, 4)"),
    "aligner_scores frame limit": "ValueError: aligner_scores: 4097 frames and 3 tokens exceed the limits of 4096 frames and 1024 tokens",
    "aligner_scores frames high": "ValueError: aligner_scores: utterance 1: 6 frames and 3 tokens do not lie in [1, 5] and [1, 3]",
    "aligner_scores keys elsewhere": "ValueError: aligner_scores: queries are on cpu and keys on meta",
    "aligner_scores prior elsewhere": "ValueError: aligner_scores: queries are on cpu and log_prior on meta",
    "aligner_scores prior shape": "ValueError: aligner_scores: expected a log_prior of shape (2, 5, 3), got (2, 5, 4)",
    "aligner_scores rank": _QK % ("(5, 4)", "(2, 3, 4)"),
    "aligner_scores token limit": "ValueError: aligner_scores: 5 frames and 1025 tokens exceed the limits of 4096 frames and 1024 tokens",
    "aligner_scores tokens low": "ValueError: aligner_scores: utterance 0: 5 frames and 0 tokens do not lie in [1, 5] and [1, 3]",
    "alignment_metrics lengths": "ValueError: alignment_metrics: input_lengths must lie in [1, 3], got [4]",
    "alignment_metrics path": "ValueError: alignment_metrics: the path of utterance 0 leaves its 3 tokens",
    "alignment_metrics shapes": "ValueError: alignment_metrics: expected (B, To, Ti) alignments and a (B, To) path, got (2, 5, 3) and (2, 4)",
    "attention_durations no tensor": "TypeError: attention_durations: expected a tensor, got list",
    "beta_binomial count": "ValueError: beta_binomial_log_prior: n_1 lengths for a batch of 2",
    "beta_binomial limit": "ValueError: beta_binomial_log_prior: 4097 frames and 3 tokens exceed the limits of 4096 frames and 1024 tokens",
    "beta_binomial none": "ValueError: beta_binomial_log_prior: expected the frames and tokens of at least one utterance",
    "beta_binomial range": "ValueError: beta_binomial_log_prior: utterance 0: 5 frames and 3 tokens do not lie in [1, 4] and [1, 3]",
    "durations_to_path count": "ValueError: durations_to_path: n_1 lengths for a batch of 2",
    "durations_to_path device count": "ValueError: durations_to_path: n_3 lengths for a batch of 2",
    "durations_to_path device rank": "ValueError: durations_to_path: n_2 lengths for a batch of 2",
    "durations_to_path dtype": "TypeError: durations_to_path: expected int32 or int64 durations, got torch.float32",
    "durations_to_path empty": "ValueError: durations_to_path: expected (B, N) or (N,) durations with at least one token, got shape (2, 0)",
    "durations_to_path lengths elsewhere": "ValueError: durations_to_path: durations are on cpu and n_lengths on meta",
    "durations_to_path no tensor": "TypeError: durations_to_path: expected int32 or int64 durations, got list",
    "durations_to_path rank": "ValueError: durations_to_path: expected (B, N) or (N,) durations with at least one token, got shape (2, 3, 4)",
    "durations_to_path token limit": "ValueError: durations_to_path: 1025 tokens exceed the limit of 1024",
    "durations_to_path tokens high": "ValueError: durations_to_path: utterance 0: 4 tokens do not lie in [0, 3]",
    "durations_to_path tokens low": "ValueError: durations_to_path: utterance 1: -1 tokens do not lie in [0, 3]",
    "length_regulate channel limit": "ValueError: length_regulate: 513 channels exceed the limit of 512",
    "length_regulate dtype": "TypeError: length_regulate: expected a float32 tensor, got torch.float64",
    "length_regulate durations dtype": "TypeError: length_regulate: expected int32 or int64 durations, got torch.float32",
    "length_regulate durations elsewhere": "ValueError: length_regulate: the tokens are on cpu and the durations on meta",
    "length_regulate durations shape": "ValueError: length_regulate: expected durations of shape (2, 3), got (2, 4)",
    "length_regulate empty": "ValueError: length_regulate: expected (B, N, C) or (N, C) tokens, got shape (2, 3, 0)",
    "length_regulate flat durations": "ValueError: length_regulate: expected (B, N) or (N,) durations with at least one token, got shape (3,)",
    "length_regulate rank": "ValueError: length_regulate: expected (B, N, C) or (N, C) tokens, got shape (2, 3, 4, 5)",
    "length_regulate tokens high": "ValueError: length_regulate: utterance 1: 4 tokens do not lie in [0, 3]",
    "ragged_conv1d batch": "ValueError: ragged_conv1d: 65536 utterances exceed the limit of 65535",
    "ragged_conv1d bias dtype": "TypeError: ragged_conv1d: expected float32 bias, got torch.float64",
    "ragged_conv1d bias elsewhere": "ValueError: ragged_conv1d: x is on cpu and bias on meta",
    "ragged_conv1d bias shape": "ValueError: ragged_conv1d: expected bias (32,), got (31,)",
    "ragged_conv1d channels in": "ValueError: ragged_conv1d: 48 input channels are not a multiple of 32, at most 4096",
    "ragged_conv1d channels out": "ValueError: ragged_conv1d: 4128 output channels are not a multiple of 32, at most 4096",
    "ragged_conv1d count": "ValueError: ragged_conv1d: 3 lengths for a batch of 2",
    "ragged_conv1d dtype": "TypeError: ragged_conv1d: expected float32 x, got torch.float64",
    "ragged_conv1d empty": "ValueError: ragged_conv1d: expected x (B, T, C), got (2, 0, 32)",
    "ragged_conv1d even": "ValueError: ragged_conv1d: a kernel width of 2 is not odd and at most 9",
    "ragged_conv1d frames": "ValueError: ragged_conv1d: 4097 frames exceed the limit of 4096",
    "ragged_conv1d frames high": "ValueError: ragged_conv1d: utterance 1: 7 frames do not lie in [0, 6]",
    "ragged_conv1d lengths elsewhere": "ValueError: ragged_conv1d: x is on cpu and lengths on meta",
    "ragged_conv1d rank": "ValueError: ragged_conv1d: expected x (B, T, C), got (6, 32)",
    "ragged_conv1d weight dtype": "TypeError: ragged_conv1d: expected float32 weight, got torch.float64",
    "ragged_conv1d weight elsewhere": "ValueError: ragged_conv1d: x is on cpu and weight on meta",
    "ragged_conv1d weight shape": "ValueError: ragged_conv1d: expected weight (Cout, 32, k), got (32, 64, 3)",
    "ragged_conv1d wide": "ValueError: ragged_conv1d: a kernel width of 11 is not odd and at most 9",
    "self_attention batch": _QKV % ("(2, 6, 2, 32)", "(1, 6, 2, 32)", "(2, 6, 2, 32)"),
    "self_attention batch heads": "ValueError: self_attention: 4096 utterances times 16 heads exceed the limit of 65535",
    "self_attention count": "ValueError: self_attention: 1 lengths for a batch of 2",
    "self_attention device count": "ValueError: self_attention: expected 2 integer lengths, got shape (3,) torch.int32",
    "self_attention device float": "ValueError: self_attention: expected 2 integer lengths, got shape (2,) torch.float32",
    "self_attention dtype k": "TypeError: self_attention: expected float32 k, got torch.float16",
    "self_attention dtype q": "TypeError: self_attention: expected float32 q, got torch.float64",
    "self_attention dtype v": "TypeError: self_attention: expected float32 v, got list",
    "self_attention empty": _QKV % (("(2, 0, 2, 32)",) * 3),
    "self_attention frames": "ValueError: self_attention: 4097 frames exceed the limit of 4096",
    "self_attention frames high": "ValueError: self_attention: utterance 1: 7 frames do not lie in [0, 6]",
    "self_attention frames low": "ValueError: self_attention: utterance 0: -1 frames do not lie in [0, 6]",
    "self_attention heads": "ValueError: self_attention: 17 heads exceed the limit of 16",
    "self_attention k elsewhere": "ValueError: self_attention: q is on cpu and k on meta",
    "self_attention lengths elsewhere": "ValueError: self_attention: q is on cpu and lengths on meta",
    "self_attention rank": _QKV % (("(6, 32)",) * 3),
    "self_attention width": "ValueError: self_attention: a head width of 48 is not one of 32, 64, 96, 128",
    "token_average batch": "ValueError: token_average: expected durations (3, N), got shape (2, 3)",
    "token_average channel limit": "ValueError: token_average: 5 frames and 513 channels exceed the limits of 65536 frames and 512 channels",
    "token_average dtype": "TypeError: token_average: expected float32 values, got torch.float64",
    "token_average durations elsewhere": "ValueError: token_average: the values are on cpu and the durations on meta",
    "token_average empty": "ValueError: token_average: expected (B, T) or (B, T, C) values, got shape (2, 0)",
    "token_average frame limit": "ValueError: token_average: 65537 frames and 1 channels exceed the limits of 65536 frames and 512 channels",
    "token_average rank": "ValueError: token_average: expected (B, T) or (B, T, C) values, got shape (5,)",
    "token_average weights dtype": "TypeError: token_average: expected float32 weights, got torch.float64",
    "token_average weights elsewhere": "ValueError: token_average: the values are on cpu and the weights on meta",
    "token_average weights shape": "ValueError: token_average: expected weights of shape (2, 5), got (2, 4)",
})


def _c(entry, text):
    return "NativeError: t2amd_%s failed (code 1): %s" % (entry, text)


_WS = "NativeError: %s: the workspace must be a contiguous uint8 tensor, got %s"
_LEN = "NativeError: %s: lengths must be a contiguous int32 vector of 2 frame counts"
_BTN = "NativeError: %s: expected a (B, T, N) tensor with unit stride along N, got shape %s stride %s"
_FULL = "NativeError: expected a contiguous tensor, got shape %s stride %s"
_ROWS = "NativeError: %s: expected contiguous %s %s, got shape %s stride %s"
_INTS = "NativeError: %s: expected contiguous int32 %s of shape %s, got %s %s"
_FSB = "NativeError: forward_sum_backward: expected grad (2, 5, 3), log_z and scale (2,) and soft (2, 3), got %s, (2,), None and %s"
NATIVE_ANSWERED = {
    "align_limits": "ok (256, 4096, 1024)",
    "align_workspace": "ok 72",
    "align_workspace empty": _c("align_workspace", "monotonic_align: 1 to 2^20 utterances: B 0 frames 5 tokens 3"),
    "align_workspace frames": _c("align_workspace", "monotonic_align: at most 4096 frames: B 2 frames 4097 tokens 3"),
    "align_workspace tokens": _c("align_workspace", "monotonic_align: at most 1024 tokens: B 2 frames 2000 tokens 1025"),
    "aligner_scores operands": "NativeError: aligner_scores: expected queries (B, T, C) and keys (B, N, C), got (2, 5, 4) and (3, 3, 4)",
    "aligner_scores prior stride": _BTN % ("aligner_scores", "(2, 5, 3)", "(15, 1, 5)"),
    "aligner_scores q stride": _FULL % ("(2, 5, 4)", "(20, 1, 5)"),
    "aligner_scores shape": "NativeError: aligner_scores: expected scores and log_prior (2, 5, 3), got (2, 5, 4) and None",
    "aligner_scores tau": _c("aligner_scores_f32", "aligner_scores: the temperature must be positive and finite"),
    "aligner_scores workspace": _WS % ("aligner_scores", "torch.int32"),
    "aligner_scores_backward kept": _WS % ("aligner_scores_backward", "torch.int32"),
    "aligner_scores_backward shapes": "NativeError: aligner_scores_backward: expected grad and dlogp (2, 5, 3), dq (2, 5, 4) and dk (2, 3, 4), "
                                      "got (2, 5, 3), None, (2, 5, 4) and (2, 3, 5)",
    "aligner_workspace": "ok (800, 848, 3360)",
    "aligner_workspace channels": _c("aligner_workspace", "aligner_workspace: 1 to 512 channels: B 2 frames 5 tokens 3 channels 513"),
    "aligner_workspace which": _c("aligner_workspace", "aligner_workspace: which must be 0 (forward), 1 (forward, kept) or 2 (backward)"),
    "beta_binomial_log_prior rank": "NativeError: beta_binomial_log_prior: expected a (B, T, N) tensor, got (5, 3)",
    "beta_binomial_log_prior stride": _FULL % ("(2, 5, 3)", "(15, 1, 5)"),
    "dtw lengths": _LEN % "dtw",
    "dtw slab": "NativeError: dtw: the predecessor slab must be a contiguous (B, rows, cols) uint8 tensor, got torch.float32 (2, 8, 8)",
    "dtw slab batch": "NativeError: dtw: the predecessor slab must be a contiguous (B, rows, cols) uint8 tensor, got torch.uint8 (3, 8, 8)",
    "dtw_backtrack slab": "NativeError: dtw_backtrack: the predecessor slab must be a contiguous (B, rows, cols) uint8 tensor, got torch.uint8 "
                          "(2, 8, 8)",
    "durations_to_path dtype": "NativeError: durations_to_path: expected (B, N) int32 or int64 durations with unit stride along N, got "
                               "torch.float32 shape (2, 3) stride (3, 1)",
    "durations_to_path ends": _INTS % ("durations_to_path", "ends", "(2, 3)", "torch.int64", "(2, 3)"),
    "durations_to_path frames": _c("durations_to_path_i32", "durations_to_path: at most 65536 frames: B 2 tokens 3 frames 65537 channels 1"),
    "durations_to_path path": _INTS % ("durations_to_path", "path", "(2, 4)", "torch.int32", "(2, 5)"),
    "durations_to_path stride": "NativeError: durations_to_path: expected (B, N) int32 or int64 durations with unit stride along N, got "
                                "torch.int32 shape (2, 3) stride (1, 2)",
    "durations_to_path t_lengths": _INTS % ("durations_to_path", "t_lengths", "(2,)", "torch.int32", "(2,)"),
    "durations_to_path totals": "NativeError: durations_to_path: expected contiguous int64 totals of shape (2,)",
    "ffb_add_ln eps": _c("ffb_add_ln_f32", "fft_block: add_ln: eps must be positive and finite"),
    "ffb_add_ln mean": _ROWS % ("ffb_add_ln", "mean", "(2, 6)", "(2, 6, 1)", "(6, 1, 1)"),
    "ffb_add_ln rank": "NativeError: ffb_add_ln: expected x (B, T, C), got (6, 32)",
    "ffb_add_ln residual": _ROWS % ("ffb_add_ln", "residual", "(2, 6, 32)", "(2, 5, 32)", "(160, 32, 1)"),
    "ffb_add_ln_backward g": _ROWS % ("ffb_add_ln_backward", "g", "(2, 6, 32)", "(2, 6, 32)", "(192, 1, 6)"),
    "ffb_add_ln_backward rank": "NativeError: ffb_add_ln_backward: expected z (B, T, C), got (6, 32)",
    "ffb_colsum dbias": _ROWS % ("ffb_colsum", "dbias", "(32,)", "(31,)", "(1,)"),
    "ffb_colsum rank": "NativeError: ffb_colsum: expected g (B, T, C), got (6, 32)",
    "ffb_colsum workspace": _WS % ("ffb_colsum", "torch.uint8"),
    "ffb_conv bias": _ROWS % ("ffb_conv", "bias", "(32,)", "(32,)", "(2,)"),
    "ffb_conv even": _c("ffb_conv_f32", "fft_block: conv: an odd kernel width from 1 to 9: B 2 frames 6 channels 32 to 32 width 2"),
    "ffb_conv image": _ROWS % ("ffb_conv", "the weight image", "(32, 96)", "(32, 95)", "(95, 1)"),
    "ffb_conv odd stride": _c("ffb_conv_f32", "fft_block: conv: x strides must be multiples of 4 floats"),
    "ffb_conv rank": "NativeError: ffb_conv: expected x (B, T, C) with unit stride along C, got shape (6, 32) stride (32, 1)",
    "ffb_conv stride": "NativeError: ffb_conv: expected x (B, T, C) with unit stride along C, got shape (2, 6, 32) stride (192, 1, 6)",
    "ffb_conv y": _ROWS % ("ffb_conv", "y", "(2, 6, 32)", "(2, 6, 32)", "(192, 1, 6)"),
    "ffb_conv y rank": _ROWS % ("ffb_conv", "the weight image", "(-1, 96)", "(32, 96)", "(96, 1)"),
    "ffb_conv_dw dw": _ROWS % ("ffb_conv_dw", "dw", "(32, 32, 3)", "(32, 3, 32)", "(96, 32, 1)"),
    "ffb_conv_dw g": _ROWS % ("ffb_conv_dw", "g", "(2, 6, 32)", "(2, 5, 32)", "(160, 32, 1)"),
    "ffb_conv_dw workspace": _WS % ("ffb_conv_dw", "torch.int32"),
    "ffb_relu_mask rank": "NativeError: ffb_relu_mask: expected g (B, T, C), got (6, 32)",
    "ffb_relu_mask y": _ROWS % ("ffb_relu_mask", "y", "(2, 6, 32)", "(2, 6, 31)", "(186, 31, 1)"),
    "fft_block_limits": "ok (4096, 4096, 9, 32, 65535)",
    "fft_block_workspace": "ok (0, 40960, 512)",
    "fft_block_workspace channels": _c("fft_block_workspace", "fft_block: workspace: input channels must be a multiple of 32, at most 4096: "
                                                              "B 2 frames 6 channels 4128 to 64 width 3"),
    "fft_block_workspace kernel": _c("fft_block_workspace", "fft_block: workspace: an odd kernel width from 1 to 9: B 2 frames 6 channels 32 "
                                                            "to 64 width 4"),
    "forward_sum lengths": _LEN % "forward_sum",
    "forward_sum log_z": "NativeError: forward_sum: expected log_z (2,), got (3,)",
    "forward_sum rank": _BTN % ("forward_sum", "(5, 3)", "(3, 1)"),
    "forward_sum workspace": _WS % ("forward_sum", "torch.int8"),
    "forward_sum_backward grad shape": _FSB % ("(2, 5, 4)", "None"),
    "forward_sum_backward grad stride": _BTN % ("forward_sum_backward", "(2, 5, 3)", "(15, 1, 5)"),
    "forward_sum_backward soft": _FSB % ("(2, 5, 3)", "(2, 4)"),
    "forward_sum_backward workspace": _WS % ("forward_sum_backward", "torch.uint8"),
    "forward_sum_workspace": "ok (272, 32)",
    "forward_sum_workspace frames": _c("forward_sum_workspace", "forward_sum: at most 4096 frames: B 2 frames 4097 tokens 3"),
    "length_regulate channels": _c("length_regulate_f32", "length_regulate: 1 to 512 channels: B 2 tokens 3 frames 5 channels 513"),
    "length_regulate path": _INTS % ("length_regulate", "path", "(2, 5)", "torch.int64", "(2, 5)"),
    "length_regulate stride": "NativeError: length_regulate: expected (B, rows, C) tokens with unit stride along C, got shape (2, 3, 4) stride "
                              "(12, 1, 3)",
    "length_regulate y": "NativeError: length_regulate: expected y (2, T, 4) and path (2, T), got (2, 5, 3) and (2, 5)",
    "length_regulate_backward dx": "NativeError: length_regulate_backward: expected dx (2, N, 4), got (3, 3, 4)",
    "length_regulate_backward ends": _INTS % ("length_regulate_backward", "ends", "(2, 3)", "torch.int32", "(2, 4)"),
    "length_regulate_backward rank": "NativeError: length_regulate_backward: expected (B, rows, C) gradient with unit stride along C, got shape "
                                     "(5, 4) stride (4, 1)",
    "mel_cepstrum lengths": _LEN % "mel_cepstrum",
    "mel_cepstrum stride": "NativeError: mel_cepstrum: shape mismatch mel=(2, 8, 5) stride (40, 1, 8) basis=(3, 8) out=(2, 5, 3)",
    "monotonic_align durations": "NativeError: monotonic_align: expected durations (2, 3), score (2,) and path (2, 5), got (2, 4), (2,) and None",
    "monotonic_align expanded": _c("monotonic_align_f32", "monotonic_align: score strides shorter than the matrix"),
    "monotonic_align lengths count": _LEN % "monotonic_align",
    "monotonic_align lengths dtype": _LEN % "monotonic_align",
    "monotonic_align path": "NativeError: monotonic_align: expected durations (2, 3), score (2,) and path (2, 5), got (2, 3), (2,) and (2, 4)",
    "monotonic_align rank": "NativeError: monotonic_align: expected (B, T, N) scores with unit stride along N, got shape (5, 3) stride (3, 1)",
    "monotonic_align stride": "NativeError: monotonic_align: expected (B, T, N) scores with unit stride along N, got shape (2, 5, 3) stride "
                              "(15, 1, 5)",
    "monotonic_align workspace dtype": _WS % ("monotonic_align", "torch.float32"),
    "monotonic_align workspace small": _c("monotonic_align_f32", "monotonic_align: the workspace is smaller than t2amd_align_workspace asks for"),
    "monotonic_align workspace stride": _WS % ("monotonic_align", "torch.uint8"),
    "regulate_limits": "ok (512, 1024, 65536)",
    "self_attn k shape": "NativeError: self_attn: expected k (B, T, H, D) = (2, 6, 2, 32) with unit stride along D, got shape (2, 5, 2, 32) "
                         "stride (320, 64, 32, 1)",
    "self_attn lengths": _LEN % "self_attn",
    "self_attn lse": _ROWS % ("self_attn", "lse", "(2, 2, 6)", "(2, 2, 6)", "(12, 1, 2)"),
    "self_attn o stride": _FULL % ("(2, 6, 2, 32)", "(384, 32, 192, 1)"),
    "self_attn odd stride": _c("self_attn_f32", "self_attn: forward: q strides must be multiples of 4 floats"),
    "self_attn rank": "NativeError: self_attn: expected q (B, T, H, D) with unit stride along D, got shape (2, 6, 32) stride (192, 32, 1)",
    "self_attn scale": _c("self_attn_f32", "self_attn: forward: the scale must be positive and finite"),
    "self_attn stride": "NativeError: self_attn: expected q (B, T, H, D) with unit stride along D, got shape (2, 6, 2, 32) stride "
                        "(384, 64, 1, 2)",
    "self_attn unaligned": _c("self_attn_f32", "self_attn: forward: q is not aligned to 16 bytes"),
    "self_attn width": _c("self_attn_f32", "self_attn: forward: a head width of 32, 64, 96 or 128: B 1 frames 2 heads 1 width 48"),
    "self_attn_backward dq": _FULL % ("(2, 6, 2, 32)", "(384, 32, 192, 1)"),
    "self_attn_backward small": _c("self_attn_bwd_f32", "self_attn: backward: the workspace is smaller than t2amd_self_attn_workspace asks for"),
    "self_attn_backward workspace": _WS % ("self_attn_backward", "torch.int32"),
    "self_attn_delta delta": _ROWS % ("self_attn_delta", "delta", "(2, 2, 6)", "(2, 6, 2)", "(12, 2, 1)"),
    "self_attn_delta o": "NativeError: self_attn_delta: expected o (B, T, H, D) = (2, 6, 2, 32) with unit stride along D, got shape "
                         "(2, 5, 2, 32) stride (320, 64, 32, 1)",
    "self_attn_limits": "ok (4096, 16, 32, 128, 65535)",
    "self_attn_workspace": "ok (0, 240, 240)",
    "self_attn_workspace heads": _c("self_attn_workspace", "self_attn: workspace: 1 to 16 heads: B 3 frames 10 heads 17 width 32"),
    "self_attn_workspace width": _c("self_attn_workspace", "self_attn: workspace: a head width of 32, 64, 96 or 128: B 3 frames 10 heads 2 "
                                                           "width 48"),
    "token_average mean": "NativeError: token_average: expected mean and num (2, N, 4) and den (2, N), got (2, 3, 4), None and (2, 4)",
    "token_average values": "NativeError: token_average: expected (B, rows, C) values with unit stride along C, got shape (2, 5, 4) stride "
                            "(20, 1, 5)",
    "token_average weights": "NativeError: token_average: expected (2, 5) weights with unit stride along T, got shape (2, 5) stride (1, 2)",
    "token_average_backward path": _INTS % ("token_average_backward", "path", "(2, 5)", "torch.int32", "(2, 6)"),
    "token_average_backward shapes": "NativeError: token_average_backward: expected grad (B, N, C), den (B, N) and dv (B, T, C), got (2, 3, 4), "
                                     "(2, 4) and (2, 5, 4)",
    "yin lengths": _LEN % "yin",
}

_SA = "* 384 64 32 * 384 64 32 * 384 64 32"
_PK = "* 1152 192 32 * 1152 192 32 * 1152 192 32"
CALLED = {
    "AlignerScores prior": ["beta_binomial_log_prior_f32(* * 2 5 3 0.5 * NULL)", "aligner_workspace(2 5 3 4 0 *)",
                            "aligner_scores_f32(* * * * 2 5 3 4 0.001 * 15 3 * 15 3 0 * 800 NULL)"],
    "FFTransformer": [
        "self_attn_f32(" + _PK + " * 2 6 2 32 0.17677669529663687 * * NULL)",
        "ffb_conv_f32(* 384 64 * * NULL * 2 6 64 96 3 1 * NULL)",
        "ffb_conv_f32(* 576 96 * * NULL * 2 6 96 64 1 0 * NULL)",
        "ffb_add_ln_f32(* * * * * 2 6 64 1e-05 * * * * NULL)",
        "ffb_add_ln_bwd_f32(* * * * * * 2 6 64 * NULL)",
        "fft_block_workspace(2 6 64 64 1 2 *)",
        "ffb_colsum_f32(* * * * * 2 6 64 * * * 512 NULL)",
        "ffb_conv_f32(* 384 64 * NULL NULL * 2 6 64 96 1 0 * NULL)",
        "fft_block_workspace(2 6 96 64 1 1 *)",
        "ffb_conv_dw_f32(* * 576 96 * 2 6 96 64 1 * * 40960 NULL)",
        "fft_block_workspace(2 6 64 64 1 2 *)",
        "ffb_colsum_f32(* NULL NULL NULL * 2 6 64 * NULL * 512 NULL)",
        "ffb_relu_mask_f32(* * * 2 6 96 * NULL)",
        "ffb_conv_f32(* 576 96 * NULL NULL * 2 6 96 64 3 0 * NULL)",
        "fft_block_workspace(2 6 64 96 3 1 *)",
        "ffb_conv_dw_f32(* * 384 64 * 2 6 64 96 3 * * 98304 NULL)",
        "fft_block_workspace(2 6 96 96 1 2 *)",
        "ffb_colsum_f32(* NULL NULL NULL * 2 6 96 * NULL * 768 NULL)",
        "self_attn_workspace(2 6 2 32 2 *)",
        "self_attn_bwd_f32(" + _PK + " * * * 384 64 32 * 2 6 2 32 0.17677669529663687 * * * * 96 NULL)"],
    "ForwardSumLoss": ["forward_sum_workspace(2 5 3 1 *)", "forward_sum_f32(* 15 3 * * 2 5 3 * 1 * 272 NULL)",
                       "forward_sum_bwd_f32(* 15 3 * * 2 5 3 * * * 15 3 NULL * 272 NULL)"],
    "LengthRegulator": ["durations_to_path_i32(* 4 1 NULL 1 1 9 * * NULL NULL NULL)", "length_regulate_f32(* 1 1 * 1 1 9 1 * NULL)"],
    "add_layer_norm backward": ["ffb_add_ln_f32(* * * * * 2 6 32 0.001 * * * * NULL)", "ffb_add_ln_bwd_f32(* * * * * * 2 6 32 * NULL)",
                                "fft_block_workspace(2 6 32 32 1 2 *)", "ffb_colsum_f32(* * * * * 2 6 32 * * * 256 NULL)"],
    "add_layer_norm plain": ["ffb_add_ln_f32(* NULL NULL NULL NULL 2 6 32 1e-05 * NULL NULL NULL NULL)"] * 2,
    "align one utterance": ["align_workspace(1 5 3 *)", "monotonic_align_f32(* 30 6 * * 1 5 3 * * NULL * 40 NULL)"],
    "align ones": ["align_workspace(1 1 1 *)", "monotonic_align_f32(* 1 1 * * 1 1 1 * * * * 24 NULL)"],
    "align ragged": ["align_workspace(2 5 3 *)", "monotonic_align_f32(* 15 3 * * 2 5 3 * * NULL * 72 NULL)"],
    "align shorter": ["align_workspace(2 5 3 *)", "monotonic_align_f32(* 48 6 * * 2 5 3 * * * * 72 NULL)"],
    "align slice": ["align_workspace(2 5 3 *)", "monotonic_align_f32(* 48 6 * * 2 5 3 * * NULL * 72 NULL)"],
    "align transposed": ["align_workspace(2 5 3 *)", "monotonic_align_f32(* 15 3 * * 2 5 3 * * NULL * 72 NULL)"],
    "aligner expanded": ["aligner_workspace(2 5 3 4 1 *)", "aligner_scores_f32(* * * * 2 5 3 4 0.5 * 15 3 * 15 3 1 * 848 NULL)",
                         "aligner_workspace(2 5 3 4 2 *)",
                         "aligner_scores_bwd_f32(* * * * 2 5 3 4 0.5 * 15 3 * * * 15 3 * 848 * 3360 NULL)"],
    "aligner more tokens": ["aligner_workspace(2 3 7 40 0 *)", "aligner_scores_f32(* * * * 2 3 7 40 0.0005 * 21 7 * 21 7 0 * 3648 NULL)"],
    "aligner ones": ["aligner_workspace(1 1 1 4 1 *)", "aligner_scores_f32(* * * * 1 1 1 4 0.0005 NULL 0 0 * 1 1 1 * 160 NULL)",
                     "aligner_workspace(1 1 1 4 2 *)",
                     "aligner_scores_bwd_f32(* * * * 1 1 1 4 0.0005 * 1 1 * * NULL 0 0 * 160 * 1168 NULL)"],
    "alignment_posterior": ["forward_sum_workspace(2 5 3 1 *)", "forward_sum_f32(* 15 3 * * 2 5 3 * 1 * 272 NULL)",
                            "forward_sum_bwd_f32(* 15 3 * * 2 5 3 * NULL * 15 3 * * 272 NULL)"],
    "durations_to_path": ["durations_to_path_i32(* 8 3 * 4 3 7 * * NULL NULL NULL)"],
    "durations_to_path one": ["durations_to_path_i32(* 4 1 NULL 1 1 0 * * NULL NULL NULL)"],
    "forward_sum backward": ["forward_sum_workspace(2 5 3 1 *)", "forward_sum_f32(* 48 6 * * 2 5 3 * 1 * 272 NULL)",
                             "forward_sum_bwd_f32(* 48 6 * * 2 5 3 * * * 48 6 NULL * 272 NULL)"],
    "forward_sum one frame": ["forward_sum_workspace(3 1 1 1 *)", "forward_sum_f32(* 1 1 * * 3 1 1 * 1 * 120 NULL)",
                              "forward_sum_bwd_f32(* 1 1 * * 3 1 1 * * * 1 1 NULL * 120 NULL)"],
    "length_regulate": ["durations_to_path_i32(* 4 3 * 2 3 7 * * * NULL NULL)", "length_regulate_f32(* 12 4 * 2 3 7 4 * NULL)",
                        "length_regulate_bwd_f32(* 28 4 * 2 3 7 4 * NULL)"],
    "length_regulate no frames": ["durations_to_path_i32(* 4 3 NULL 1 3 0 NULL * * NULL NULL)"],
    "length_regulate slice": ["durations_to_path_i32(* 4 5 NULL 2 3 1 * * NULL NULL NULL)", "length_regulate_f32(* 48 6 * 2 3 1 4 * NULL)"],
    "ragged_conv1d backward": ["ffb_conv_f32(* 192 32 * * NULL * 2 6 32 64 5 1 * NULL)", "ffb_relu_mask_f32(* * * 2 6 64 * NULL)",
                               "ffb_conv_f32(* 384 64 * NULL NULL * 2 6 64 32 5 0 * NULL)", "fft_block_workspace(2 6 32 64 5 1 *)",
                               "ffb_conv_dw_f32(* * 192 32 * 2 6 32 64 5 * * 57344 NULL)", "fft_block_workspace(2 6 64 64 1 2 *)",
                               "ffb_colsum_f32(* NULL NULL NULL * 2 6 64 * NULL * 512 NULL)"],
    "ragged_conv1d slice": ["ffb_conv_f32(* 512 64 * NULL NULL NULL 2 6 32 32 3 0 * NULL)"],
    "ragged_conv1d transposed": ["ffb_conv_f32(* 0 0 * NULL NULL NULL 1 1 32 32 1 0 * NULL)"],
    "self_attention backward": ["self_attn_f32(" + _SA + " * 2 6 2 32 0.5 * * NULL)", "self_attn_workspace(2 6 2 32 2 *)",
                                "self_attn_bwd_f32(" + _SA + " * * * 384 64 32 * 2 6 2 32 0.5 * * * * 96 NULL)"],
    "self_attention ones": ["self_attn_f32(* 0 0 0 * 0 0 0 * 0 0 0 NULL 1 1 1 32 0.17677669529663687 * NULL NULL)"],
    "self_attention packed": ["self_attn_f32(" + _PK + " * 2 6 2 32 0.17677669529663687 * NULL NULL)", "read in place: [True, True, True]"],
    "self_attention transposed": ["self_attn_f32(* 768 64 384 * 768 128 64 * 1536 256 128 NULL 2 6 2 64 0.125 * NULL NULL)"],
    "token_average": ["durations_to_path_i32(* 4 3 * 2 3 5 * * * NULL NULL)", "token_average_f32(* 5 1 * 5 * 2 3 5 1 * * NULL NULL)",
                      "token_average_bwd_f32(* * * 5 * 2 3 5 1 * NULL)"],
    "token_average channels": ["durations_to_path_i32(* 4 3 NULL 2 3 5 * * * NULL NULL)", "token_average_f32(* 20 4 * 8 * 2 3 5 4 * * NULL NULL)",
                               "token_average_bwd_f32(* * * 8 * 2 3 5 4 * NULL)"],
    "unaligned": ["self_attn_f32(" + _SA + " NULL 2 6 2 32 0.17677669529663687 * NULL NULL)",
                  "ffb_conv_f32(* 192 32 * NULL NULL NULL 2 6 32 32 3 0 * NULL)",
                  "ffb_add_ln_f32(* NULL NULL NULL NULL 2 6 32 1e-05 * NULL NULL NULL NULL)",
                  "copied: [True, True]; every pointer on 16 bytes: True"],
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_public_refusals_keep_their_type_and_text(dry, name):
    assert outcome(REFUSALS[name]) == REFUSED[name]


@pytest.mark.parametrize("name", sorted(HOST_REFUSALS))
def test_host_tensors_are_refused_in_each_modules_words(native_lib, name):
    assert not nv.validate_only()
    assert outcome(HOST_REFUSALS[name]) == HOST_REFUSED[name]


@pytest.mark.parametrize("name", sorted(NATIVE))
def test_native_wrappers_keep_their_answers(dry, name):
    assert outcome(NATIVE[name]) == NATIVE_ANSWERED[name]


@pytest.mark.parametrize("name", sorted(CALLS))
def test_good_calls_hand_c_the_same_arguments(dry, name):
    assert recorded(CALLS[name]) == CALLED[name]


def test_the_tables_cover_each_other():
    assert set(REFUSALS) == set(REFUSED) and set(HOST_REFUSALS) == set(HOST_REFUSED)
    assert set(NATIVE) == set(NATIVE_ANSWERED) and set(CALLS) == set(CALLED)
