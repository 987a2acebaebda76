"""The host layer the WaveGlow, HiFi-GAN and Vocos modules share (the device side of the same sharing is csrc/rowmma.h):
the precision / dtype switches, loading, the packed-row map and its one-entry cache, the key of the packed weight image
and the argument checks at the head of ``infer``.  Geometry, weight layouts and launch sequences stay with each model.
DESIGN.md section 11 has the split.
"""
import numpy as np
import torch
from torch import nn

from . import native as nv

PRECISIONS = {'fp32': 0, 'bf16x3': 1, 'bf16': 2}
MEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def packed_rows(rows, halo, slots=None):
    """(rowb, rowr, offsets, P) of a packed row space (int32 host tensors): ``halo`` marked rows, then per utterance b its
    ``rows[b]`` real rows (rowb = b, rowr = 0 .. rows[b] - 1) followed by ``slots[b] - rows[b] + halo`` marked rows
    (rowb = -1, rowr = 0).  ``slots`` defaults to ``rows``; offsets[b] is the first real row of utterance b."""
    rows = [int(r) for r in rows]
    slots = rows if slots is None else [int(s) for s in slots]
    rowb, rowr, offs, pos = [np.full(halo, -1, np.int32)], [np.zeros(halo, np.int32)], [], halo
    for b, (R, S) in enumerate(zip(rows, slots)):
        pad = S - R + halo
        offs.append(pos)
        rowb += [np.full(R, b, np.int32), np.full(pad, -1, np.int32)]
        rowr += [np.arange(R, dtype=np.int32), np.zeros(pad, np.int32)]
        pos += R + pad
    return torch.from_numpy(np.concatenate(rowb)), torch.from_numpy(np.concatenate(rowr)), offs, pos


def host_lengths(lengths, B, full):
    """``lengths`` (a tensor, a sequence or None: ``full`` for each of the B utterances) as a host list of ints."""
    if lengths is None:
        return [full] * B
    return [int(v) for v in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]


def checkpoint_source(src, key):
    """What a ``load_*`` function was given, opened: a path is loaded, a wrapper dict ``{key: state dict or module}`` gives
    its entry."""
    if isinstance(src, str):
        src = torch.load(src, map_location='cpu', weights_only=False)
    if isinstance(src, dict) and key in src and not torch.is_tensor(src[key]):
        src = src[key]
    return src


def _splitk(M, N, K):
    """Split count of a weight-gradient product [M][N] over K rows: about two workgroups of 128 x 128 per compute unit,
    at least 512 rows per slice."""
    tiles = -(-M // 128) * -(-N // 128)
    return max(1, min(-(-512 // tiles), K // 512, 64))


def _wgrad(out, A, Bm, prec, partials):
    """out [M][N] = A^T . Bm over the rows of A [K][M] and Bm [K][N] (halo rows are zero in one of them), split-K in a
    fixed order."""
    K, M = A.shape
    s = _splitk(M, Bm.shape[1], K)
    if s == 1:
        nv.gemm(out, A, Bm, a_km=True, b_kn=True, fast=prec)
    else:
        nv.gemm(out, A, Bm, a_km=True, b_kn=True, splitk=s, partials=partials, fast=prec)
        nv.splitk_reduce2d(partials, s, out)


class Vocoder(nn.Module):
    """Base of the three vocoder modules.  ``LABEL`` names the model in every error text; a subclass has ``n_mel_channels``
    and ``from_state_dict(state_dict, precision, ...)``."""
    LABEL = 'Vocoder'

    def __init__(self):
        super().__init__()                          # a subclass sets ``precision`` once its geometry checks have passed
        self.half_io = False
        self._pack = self._plan_cache = None

    # ---- precision / dtype -------------------------------------------------------------------------------------------
    @property
    def precision(self):
        return self._precision

    @precision.setter
    def precision(self, p):
        if p not in PRECISIONS:
            raise ValueError("%s: precision must be one of %s, got %r" % (self.LABEL, sorted(PRECISIONS), p))
        self._precision = p

    def half(self):
        """f32 master weights kept; bf16 compute, float16 output."""
        self.precision, self.half_io = 'bf16', True
        return self

    def float(self):
        super().float()
        self.precision, self.half_io = 'fp32', False
        return self

    def _io(self, out):
        return out.half() if self.half_io else out

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self._pack = self._plan_cache = None
        return self

    # ---- loading ------------------------------------------------------------------------------------------------------
    @classmethod
    def from_module(cls, module, *args, **kw):
        """Adopt a loaded reference module: its weights are read once; the other arguments are ``from_state_dict``'s."""
        with torch.no_grad():
            sd = {k: v.detach().float().cpu() for k, v in module.state_dict().items()}
        return cls.from_state_dict(sd, *args, **kw)

    @classmethod
    def _from_source(cls, src, who, **kw):
        """An opened ``checkpoint_source``: an instance as it is, a module or a state dict adopted."""
        if isinstance(src, cls):
            return src
        if isinstance(src, nn.Module):
            return cls.from_module(src, **kw)
        if isinstance(src, dict):
            return cls.from_state_dict(src, **kw)
        raise TypeError("%s: expected a path, a state dict or a module, got %s" % (who, type(src).__name__))

    @staticmethod
    def _f32_state(sd):
        return {k: v.float() if torch.is_tensor(v) and v.is_floating_point() else v for k, v in sd.items()}

    # ---- caches -------------------------------------------------------------------------------------------------------
    def _cached_plan(self, key, build):
        """``build()`` once while ``key`` repeats (one entry).  ``key`` holds everything the plan depends on."""
        if self._plan_cache is None or self._plan_cache[0] != key:
            self._plan_cache = (key, build())
        return self._plan_cache[1]

    def _pack_key(self, device):
        """What the packed weight image depends on.  torch's version counters see in-place edits and optimiser steps;
        FusedAdam and ``param.data`` edits write through raw pointers and bump the engine's weight generation instead.
        One walk over the modules' own tables: ``parameters()`` and ``buffers()`` walk the tree twice and build every dotted
        name on the way, which took 2.6 times as long for the published WaveGlow.  A shared tensor appears twice here,
        which a key does not mind."""
        from .engine import _PACK_GEN
        return (_PACK_GEN[0], str(device), tuple((t.data_ptr(), t._version) for m in self.modules()
                                                 for d in (m._parameters, m._buffers) for t in d.values() if t is not None))

    # ---- the head of a call -------------------------------------------------------------------------------------------
    def _device(self):
        dev = next(self.parameters()).device
        if dev.type != 'cuda' and not nv.validate_only():
            raise nv.NativeError("%s: move the module to the MI355X first (.cuda()); there is no CPU path" % self.LABEL)
        return dev

    def _check_mels(self, mel, lengths, who):
        """-> (B, n_mel, N, frames per utterance as a host list) of (B, n_mel, N) mels."""
        if not torch.is_tensor(mel) or mel.dim() != 3 or mel.shape[1] != self.n_mel_channels:
            raise ValueError("%s.%s: expected (B, %d, N) mels, got %s"
                             % (self.LABEL, who, self.n_mel_channels, tuple(mel.shape) if torch.is_tensor(mel) else type(mel)))
        if mel.dtype not in MEL_DTYPES:
            raise ValueError("%s.%s: mels must be float32, float16 or bfloat16, got %s" % (self.LABEL, who, mel.dtype))
        B, nm, N = mel.shape
        lens = host_lengths(lengths, B, N)
        if B < 1 or len(lens) != B or min(lens) < 1 or max(lens) > N:
            raise ValueError("%s.%s: lengths %s do not fit %d utterances of %d frames" % (self.LABEL, who, lens, B, N))
        return B, nm, N, lens

    def _check_free(self, dev, floats, workspace, P, who):
        """Refuse a call whose allocations (``floats`` float32 in all, ``workspace`` of them for P packed frames) do not
        fit."""
        if dev.type == 'cuda':
            free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
            if 4 * floats > free:
                raise nv.NativeError("%s.%s: the workspace needs %.2f GB (%d packed frames) and %.2f GB are free; split the "
                                     "batch" % (self.LABEL, who, 4 * workspace / 1e9, P, free / 1e9))

    @staticmethod
    def _regions(ws, P, widths):
        """One workspace allocation sliced into consecutive ``[P][width]`` regions."""
        out, pos = [], 0
        for w in widths:
            out.append(ws[pos:pos + P * w].view(P, w))
            pos += P * w
        return out
