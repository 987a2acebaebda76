"""The host layer the alignment, regulator and Transformer ops share above ``native`` (alignment.py, transformer.py; the native
side of the same sharing is the argument helpers beside ``native._pair_lengths``, the C side the host helpers at the foot of
csrc/common.h).  All of these ops take a padded batch, per-utterance lengths and a few strided float32 operands, so what is
shared is the plumbing: the float32 and positive-number checks, the validation of (frames, tokens) length pairs, lengths that
come as a host list or as a device tensor, their upload, the two ways a tensor is made readable for a kernel, the workspace
allocation and the "no CPU path" refusal.  Every refusal keeps the words its op has always used, so the words are arguments.
Shapes, limits, the autograd functions, what is kept for a backward and the launch sequences stay with each op.  DESIGN.md
section 18 has the split.
"""
import torch

from . import native as nv
from .audio import _lengths, _require_device

FRAMES = ("frames", "", True)        # how an op speaks of its lengths: the noun, the prefix of "lengths", and whether a device
TOKENS = ("tokens", "n_", False)     # tensor of floats is refused (the regulator converts one)


def float32(who, t, name=None):
    """TypeError unless ``t`` is a float32 tensor; ``name`` is how the text calls it ("a float32 tensor" where None)."""
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise TypeError("%s: expected %s, got %s" % (who, "float32 " + name if name else "a float32 tensor",
                                                     t.dtype if torch.is_tensor(t) else type(t).__name__))


def positive(who, v, text, bools=True, cap=float("inf")):
    """``v`` as a float: a positive finite int or float, at most ``cap``; ``bools`` False refuses True as well.  ``text`` says
    what must hold."""
    if not isinstance(v, (int, float)) or (isinstance(v, bool) and not bools) or not (0.0 < float(v) <= cap and float(v) < float("inf")):
        raise ValueError("%s: %s, got %r" % (who, text, v))
    return float(v)


def require_device(t, who=None, what=None):
    """NativeError for a host tensor outside validate-only mode: in ``audio``'s words, or with ``who`` in the Transformer ops'
    ("x is", "q, k and v are")."""
    if who is None:
        return _require_device(t)
    if not t.is_cuda and not nv.validate_only():
        raise nv.NativeError("%s: %s on %s; move %s to the MI355X first, there is no CPU path"
                             % (who, what, t.device, "them" if what.endswith("are") else "it"))


def path_lengths(who, t_lengths, n_lengths, B, T, N, limits, monotonic=False):
    """The frames and tokens of B utterances in a (B, T, N) buffer as two host lists (the buffer's own where None), each within
    [1, T] and [1, N].  ``limits`` = (frames, tokens) at most: of the buffer, or with ``monotonic`` of every utterance, which
    then also needs N_b <= T_b."""
    tl = _lengths(t_lengths, B, None, who + ": t_", full=T)
    nl = _lengths(n_lengths, B, None, who + ": n_", full=N)
    for b in range(B):
        if not (1 <= tl[b] <= T and 1 <= nl[b] <= N):
            raise ValueError("%s: utterance %d: %d frames and %d tokens do not lie in [1, %d] and [1, %d]" % (who, b, tl[b], nl[b], T, N))
        if monotonic and (tl[b] > limits[0] or nl[b] > limits[1]):
            raise ValueError("%s: utterance %d: %d frames and %d tokens exceed the limits of %d frames and %d tokens"
                             % ((who, b, tl[b], nl[b]) + tuple(limits)))
        if monotonic and nl[b] > tl[b]:
            raise ValueError("%s: utterance %d has %d tokens and only %d frames; a monotonic path needs 1 <= N <= T" % (who, b, nl[b], tl[b]))
    if not monotonic and (T > limits[0] or N > limits[1]):
        raise ValueError("%s: %d frames and %d tokens exceed the limits of %d frames and %d tokens" % ((who, T, N) + tuple(limits)))
    return tl, nl


def upload(dev, *lists):
    """Host lists of lengths as int32 tensors on ``dev``."""
    return tuple(torch.tensor(v, dtype=torch.int32).to(dev) for v in lists)


def device_lengths(who, lengths, B, hi, dev, owner, kind=FRAMES):
    """Per-utterance counts as an int32 vector on ``dev``, or None.  A host list is checked against [0, hi] and uploaded; a device
    tensor is not read here: the kernels clamp it.  ``owner`` is how the text names what lies on ``dev`` ("q is", "durations
    are"), ``kind`` is FRAMES or TOKENS."""
    noun, prefix, integers = kind
    if lengths is None:
        return None
    if torch.is_tensor(lengths) and lengths.device.type != "cpu":
        if lengths.device != dev:
            raise ValueError("%s: %s on %s and %slengths on %s" % (who, owner, dev, prefix, lengths.device))
        if lengths.dim() != 1 or lengths.numel() != B or (integers and lengths.is_floating_point()):
            raise ValueError("%s: expected %d integer lengths, got shape %s %s" % (who, B, tuple(lengths.shape), lengths.dtype) if integers
                             else "%s: %s%d lengths for a batch of %d" % (who, prefix, lengths.numel(), B))
        return lengths.detach().to(torch.int32).contiguous()
    ln = _lengths(lengths, B, None, "%s: %s" % (who, prefix))
    for b in range(B):
        if not 0 <= ln[b] <= hi:
            raise ValueError("%s: utterance %d: %d %s do not lie in [0, %d]" % (who, b, ln[b], noun, hi))
    return upload(dev, ln)[0]


def dense_rows(x):
    """``x`` (B, T, N) as the path, aligner and regulator kernels take it: unit stride along N and row and batch strides that
    cover the matrix (an expanded or transposed tensor is copied)."""
    B, T, N = x.shape
    ok = x.stride(2) == 1 and (T == 1 or x.stride(1) >= N) and (B == 1 or x.stride(0) >= (T - 1) * max(x.stride(1), N) + N)
    return x if ok else x.contiguous()


def aligned(x, strided=True):
    """``x`` as the matrix-pipe kernels take it, read as it is where that can be and copied onto 16 bytes where not: unit stride
    along the last axis, the other strides positive multiples of 4 floats (so the chunks of a packed projection pass), the base
    on 16 bytes; without ``strided`` nothing but a contiguous tensor passes."""
    n = x.dim() - 1
    ok = x.stride(n) == 1 and all(x.shape[i] == 1 or (x.stride(i) > 0 and x.stride(i) % 4 == 0) for i in range(n)) if strided \
        else x.is_contiguous()
    if not ok:
        x = x.contiguous()
    return x if x.data_ptr() % 16 == 0 else x.clone(memory_format=torch.contiguous_format)


def workspace(nbytes, dev, least=0):
    """A uint8 workspace of ``nbytes`` on ``dev``, of ``least`` bytes where the query asks for fewer."""
    return torch.empty(max(int(nbytes), least), dtype=torch.uint8, device=dev)
