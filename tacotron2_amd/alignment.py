"""Forced alignment on the GPU: the best monotonic path through a (frames, tokens) score matrix (csrc/align.hip, DESIGN.md
section 18; Glow-TTS's "monotonic alignment search"), per-token durations from a Tacotron 2 attention matrix, and what the
attention did beside that path; and the sum over all such paths (csrc/forward_sum.hip; the forward-sum
alignment likelihood of "One TTS Alignment To Rule Them All") with its gradient, the posterior occupancy of every cell; and the
scores a learned aligner feeds both with (csrc/aligner.hip, csrc/aligner_rows.hip): the distances between
projected frames and projected tokens, normalised over the tokens, plus a beta-binomial prior, with their gradient.

    durations, score = monotonic_align(scores, t_lengths, n_lengths)
    durations, score, path = attention_durations(alignments, input_lengths, output_lengths, return_path=True)
    metrics = alignment_metrics(alignments, path, input_lengths, output_lengths)
    log_z = forward_sum(scores, t_lengths, n_lengths)                      # differentiable: d log_z / d scores = gamma
    gamma, soft_durations, log_z = alignment_posterior(scores, t_lengths, n_lengths)
    loss = ForwardSumLoss(reduction='mean', per_frame=False)(scores, t_lengths, n_lengths)
    scores = aligner_scores(queries, keys, t_lengths, n_lengths, temperature=0.0005, log_prior=None)   # differentiable
    log_prior = beta_binomial_log_prior(t_lengths, n_lengths, scaling=1.0)
    scores = AlignerScores(temperature=0.0005, prior_scaling=1.0)(queries, keys, t_lengths, n_lengths)

``monotonic_align``, ``attention_durations``, ``alignment_metrics`` and ``beta_binomial_log_prior`` have no gradient;
``forward_sum``, ``ForwardSumLoss``, ``aligner_scores`` and ``AlignerScores`` have one.  There is no CPU path."""
import numpy as np
import torch

from . import native as nv
from .audio import _lengths, _require_device

MAX_FRAMES = 4096
MAX_TOKENS = 1024
MAX_CHANNELS = 512
METRIC_KEYS = ("focus", "path_mass", "off_path", "backward_steps", "max_duration")


@torch.no_grad()
def monotonic_align(scores, t_lengths=None, n_lengths=None, return_path=False):
    """The admissible path n(0) = 0, n(T-1) = N-1, n(t) - n(t-1) in {0, 1} of greatest summed score through each utterance of
    the float32 device tensor ``scores`` (B, T, N) or (T, N): Q(t,n) = scores(t,n) + max(Q(t-1,n), Q(t-1,n-1)) in float32, staying
    wins ties.  ``t_lengths`` / ``n_lengths`` are the frames and tokens of every utterance (the buffer's own where None); each
    utterance needs 1 <= N <= T, T <= 4096, N <= 1024.  -> ``durations`` (B, N) int32, the frames on each token (zeros at and
    beyond an utterance's N; a row sums to its T), ``score`` (B,) float32 = Q(T-1, N-1), and with ``return_path`` also ``path``
    (B, T) int32, the token of every frame (-1 at and beyond T)."""
    if not torch.is_tensor(scores) or scores.dtype != torch.float32:
        raise TypeError("monotonic_align: expected a float32 tensor, got %s"
                        % (scores.dtype if torch.is_tensor(scores) else type(scores).__name__))
    if scores.dim() == 2:
        scores = scores.unsqueeze(0)
    if scores.dim() != 3 or min(scores.shape) < 1:
        raise ValueError("monotonic_align: expected (B, T, N) or (T, N) scores, got shape %s" % (tuple(scores.shape),))
    _require_device(scores)
    scores = scores.detach()
    B, T, N = scores.shape
    tl = _lengths(t_lengths, B, None, "monotonic_align: t_", full=T)
    nl = _lengths(n_lengths, B, None, "monotonic_align: n_", full=N)
    for b in range(B):
        if not (1 <= tl[b] <= T and 1 <= nl[b] <= N):
            raise ValueError("monotonic_align: utterance %d: %d frames and %d tokens do not lie in [1, %d] and [1, %d]"
                             % (b, tl[b], nl[b], T, N))
        if tl[b] > MAX_FRAMES or nl[b] > MAX_TOKENS:
            raise ValueError("monotonic_align: utterance %d: %d frames and %d tokens exceed the limits of %d frames and %d tokens"
                             % (b, tl[b], nl[b], MAX_FRAMES, MAX_TOKENS))
        if nl[b] > tl[b]:
            raise ValueError("monotonic_align: utterance %d has %d tokens and only %d frames; a monotonic path needs 1 <= N <= T"
                             % (b, nl[b], tl[b]))
    Tm, Nm = max(tl), max(nl)
    dev = scores.device
    s = scores[:, :Tm, :Nm]
    if Nm > 1 and s.stride(2) != 1:
        s = s.contiguous()
    t_dev, n_dev = (torch.tensor(v, dtype=torch.int32).to(dev) for v in (tl, nl))
    durations = torch.empty(B, Nm, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    path = torch.empty(B, Tm, dtype=torch.int32, device=dev) if return_path else None
    ws = torch.empty(nv.align_workspace(B, Tm, Nm), dtype=torch.uint8, device=dev)
    nv.monotonic_align(s, t_dev, n_dev, durations, score, path, ws)
    if Nm < N:                                                              # a longer buffer holding shorter utterances
        durations = torch.nn.functional.pad(durations, (0, N - Nm))
    if return_path and Tm < T:
        path = torch.nn.functional.pad(path, (0, T - Tm), value=-1)
    return (durations, score, path) if return_path else (durations, score)


@torch.no_grad()
def attention_durations(alignments, input_lengths, output_lengths, eps=1e-8, return_path=False):
    """Per-token durations from the attention matrix ``alignments`` (B, To, Ti) that ``Tacotron2.forward`` and ``.inference``
    return: ``monotonic_align`` of log(max(alignments, eps)) with ``output_lengths`` frames and ``input_lengths`` tokens."""
    if not torch.is_tensor(alignments):
        raise TypeError("attention_durations: expected a tensor, got %s" % type(alignments).__name__)
    return monotonic_align(torch.log(alignments.detach().float().clamp_min(eps)), output_lengths, input_lengths, return_path)


def alignment_metrics(alignments, path, input_lengths, output_lengths):
    """What the attention ``alignments`` (B, To, Ti) did beside the monotonic ``path`` (B, To), per utterance, in float64 on the
    host ("argmax" is the lowest index among the maxima) -> a dict of (B,) float64 arrays:
    ``focus`` the mean over frames of max_n A; ``path_mass`` the mean over frames of A[t, path[t]]; ``off_path`` the share of
    frames whose argmax is not path[t]; ``backward_steps`` the count of frames t >= 1 whose argmax lies below the previous
    frame's; ``max_duration`` the largest number of frames on one token of the path."""
    A = alignments.detach().double().cpu().numpy() if torch.is_tensor(alignments) else np.asarray(alignments, dtype=np.float64)
    P = path.detach().cpu().numpy() if torch.is_tensor(path) else np.asarray(path)
    if A.ndim == 2:
        A, P = A[None], P[None] if P.ndim == 1 else P
    if A.ndim != 3 or P.shape != A.shape[:2]:
        raise ValueError("alignment_metrics: expected (B, To, Ti) alignments and a (B, To) path, got %s and %s" % (A.shape, P.shape))
    B = A.shape[0]
    ni = _lengths(input_lengths, B, A.shape[2], "alignment_metrics: input_", full=A.shape[2])
    no = _lengths(output_lengths, B, A.shape[1], "alignment_metrics: output_", full=A.shape[1])
    out = {k: np.zeros(B, dtype=np.float64) for k in METRIC_KEYS}
    for b in range(B):
        a, p = A[b, :no[b], :ni[b]], P[b, :no[b]].astype(np.int64)
        if p.min() < 0 or p.max() >= ni[b]:
            raise ValueError("alignment_metrics: the path of utterance %d leaves its %d tokens" % (b, ni[b]))
        top = a.argmax(axis=1)
        out["focus"][b] = a.max(axis=1).mean()
        out["path_mass"][b] = a[np.arange(no[b]), p].mean()
        out["off_path"][b] = (top != p).mean()
        out["backward_steps"][b] = (top[1:] < top[:-1]).sum()
        out["max_duration"][b] = np.bincount(p).max()
    return out


def _forward_sum_args(scores, t_lengths, n_lengths):
    """The validation of ``monotonic_align`` under the prefix ``forward_sum:`` -> (scores as (B, T, N), frames, tokens)."""
    if not torch.is_tensor(scores) or scores.dtype != torch.float32:
        raise TypeError("forward_sum: expected a float32 tensor, got %s"
                        % (scores.dtype if torch.is_tensor(scores) else type(scores).__name__))
    if scores.dim() == 2:
        scores = scores.unsqueeze(0)
    if scores.dim() != 3 or min(scores.shape) < 1:
        raise ValueError("forward_sum: expected (B, T, N) or (T, N) scores, got shape %s" % (tuple(scores.shape),))
    _require_device(scores)
    B, T, N = scores.shape
    tl = _lengths(t_lengths, B, None, "forward_sum: t_", full=T)
    nl = _lengths(n_lengths, B, None, "forward_sum: n_", full=N)
    for b in range(B):
        if not (1 <= tl[b] <= T and 1 <= nl[b] <= N):
            raise ValueError("forward_sum: utterance %d: %d frames and %d tokens do not lie in [1, %d] and [1, %d]"
                             % (b, tl[b], nl[b], T, N))
        if tl[b] > MAX_FRAMES or nl[b] > MAX_TOKENS:
            raise ValueError("forward_sum: utterance %d: %d frames and %d tokens exceed the limits of %d frames and %d tokens"
                             % (b, tl[b], nl[b], MAX_FRAMES, MAX_TOKENS))
        if nl[b] > tl[b]:
            raise ValueError("forward_sum: utterance %d has %d tokens and only %d frames; a monotonic path needs 1 <= N <= T"
                             % (b, nl[b], tl[b]))
    return scores, tl, nl


def _forward_sum_launch(scores, tl, nl, keep):
    """The alpha launch over the longest utterance's part of ``scores`` -> (that part, device lengths, log_z, workspace)."""
    B = scores.shape[0]
    Tm, Nm = max(tl), max(nl)
    dev = scores.device
    s = scores.detach()[:, :Tm, :Nm]
    if Nm > 1 and s.stride(2) != 1:
        s = s.contiguous()
    t_dev, n_dev = (torch.tensor(v, dtype=torch.int32).to(dev) for v in (tl, nl))
    log_z = torch.empty(B, dtype=torch.float32, device=dev)
    ws = torch.empty(nv.forward_sum_workspace(B, Tm, Nm, keep), dtype=torch.uint8, device=dev)
    nv.forward_sum(s, t_dev, n_dev, log_z, ws, keep)
    return s, t_dev, n_dev, log_z, ws


def _forward_sum_gamma(shape, s, t_dev, n_dev, log_z, scale, ws, soft):
    """The beta launch -> scale times gamma at the buffer's own ``shape`` (zeros beyond the longest utterance)."""
    B, Tm, Nm = s.shape
    whole = tuple(shape) == (B, Tm, Nm)
    grad = (torch.empty if whole else torch.zeros)(shape, dtype=torch.float32, device=s.device)
    nv.forward_sum_backward(s, t_dev, n_dev, log_z, scale, grad[:, :Tm, :Nm], soft, ws)
    return grad


class _ForwardSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, tl, nl, keep):
        s, t_dev, n_dev, log_z, ws = _forward_sum_launch(scores, tl, nl, keep)
        if keep:
            ctx.shape = scores.shape
            ctx.save_for_backward(s, t_dev, n_dev, log_z, ws)
        return log_z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        s, t_dev, n_dev, log_z, ws = ctx.saved_tensors
        return _forward_sum_gamma(ctx.shape, s, t_dev, n_dev, log_z, grad_output.float().contiguous(), ws, None), None, None, None


def forward_sum(scores, t_lengths=None, n_lengths=None):
    """``log_z`` (B,) float32: the log of the summed probability of all admissible paths (those of ``monotonic_align``) through
    each utterance of the float32 device tensor ``scores`` (B, T, N) or (T, N): alpha(0,0) = scores(0,0), alpha(t,n) = scores(t,n)
    + logaddexp(alpha(t-1,n), alpha(t-1,n-1)), log_z = alpha(T-1, N-1).  Lengths, limits and refusals are those of
    ``monotonic_align``.  A score of -inf marks an impossible cell; an utterance without a possible path gives -inf.
    Differentiable: the gradient with respect to ``scores`` is ``grad_output`` times the posterior occupancy gamma (zeros in the
    padding).  Under ``no_grad``, or where ``scores`` does not require a gradient, nothing is kept for a backward pass."""
    scores, tl, nl = _forward_sum_args(scores, t_lengths, n_lengths)
    return _ForwardSum.apply(scores, tl, nl, torch.is_grad_enabled() and scores.requires_grad)


@torch.no_grad()
def alignment_posterior(scores, t_lengths=None, n_lengths=None):
    """-> ``gamma`` (B, T, N) float32, the posterior probability that a path drawn in proportion to exp(its score) is on token n
    at frame t (d log_z / d scores; a row within an utterance sums to 1, zeros in the padding), ``soft_durations`` (B, N) float32,
    its column sums (the expected frames on each token; a row sums to the utterance's T), and ``log_z`` (B,) as ``forward_sum``
    gives it.  An utterance without a possible path has zeros and -inf."""
    scores, tl, nl = _forward_sum_args(scores, t_lengths, n_lengths)
    s, t_dev, n_dev, log_z, ws = _forward_sum_launch(scores, tl, nl, True)
    soft = torch.empty(s.shape[0], s.shape[2], dtype=torch.float32, device=s.device)
    gamma = _forward_sum_gamma(scores.shape, s, t_dev, n_dev, log_z, None, ws, soft)
    if s.shape[2] < scores.shape[2]:                                        # a longer buffer holding shorter utterances
        soft = torch.nn.functional.pad(soft, (0, scores.shape[2] - s.shape[2]))
    return gamma, soft, log_z


class ForwardSumLoss(torch.nn.Module):
    """-log_z of ``forward_sum`` per utterance, divided by the utterance's frames where ``per_frame``, then reduced by
    ``reduction`` ('mean', 'sum' or 'none')."""

    def __init__(self, reduction='mean', per_frame=False):
        super().__init__()
        if reduction not in ('mean', 'sum', 'none'):
            raise ValueError("ForwardSumLoss: reduction must be 'mean', 'sum' or 'none', got %r" % (reduction,))
        self.reduction, self.per_frame = reduction, bool(per_frame)

    def forward(self, scores, t_lengths=None, n_lengths=None):
        scores, tl, nl = _forward_sum_args(scores, t_lengths, n_lengths)
        loss = -forward_sum(scores, tl, nl)
        if self.per_frame:
            loss = loss / torch.tensor(tl, dtype=torch.float32).to(loss.device)
        return loss if self.reduction == 'none' else loss.mean() if self.reduction == 'mean' else loss.sum()


def _aligner_lengths(who, t_lengths, n_lengths, B, T, N):
    tl = _lengths(t_lengths, B, None, who + ": t_", full=T)
    nl = _lengths(n_lengths, B, None, who + ": n_", full=N)
    for b in range(B):
        if not (1 <= tl[b] <= T and 1 <= nl[b] <= N):
            raise ValueError("%s: utterance %d: %d frames and %d tokens do not lie in [1, %d] and [1, %d]"
                             % (who, b, tl[b], nl[b], T, N))
    if T > MAX_FRAMES or N > MAX_TOKENS:
        raise ValueError("%s: %d frames and %d tokens exceed the limits of %d frames and %d tokens" % (who, T, N, MAX_FRAMES, MAX_TOKENS))
    return tl, nl


def _dense_rows(x):
    """``x`` (B, T, N) as the kernels take it: unit stride along N and row and batch strides that cover the matrix (an expanded
    or transposed tensor is copied)."""
    B, T, N = x.shape
    ok = x.stride(2) == 1 and (T == 1 or x.stride(1) >= N) and (B == 1 or x.stride(0) >= (T - 1) * max(x.stride(1), N) + N)
    return x if ok else x.contiguous()


class _AlignerScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, logp, tl, nl, tau, keep):
        B, T, C = q.shape
        N = k.shape[1]
        dev = q.device
        qd, kd = q.detach().contiguous(), k.detach().contiguous()
        lp = None if logp is None else _dense_rows(logp.detach())
        t_dev, n_dev = (torch.tensor(v, dtype=torch.int32).to(dev) for v in (tl, nl))
        scores = torch.empty(B, T, N, dtype=torch.float32, device=dev)
        ws = torch.empty(nv.aligner_workspace(B, T, N, C, 1 if keep else 0), dtype=torch.uint8, device=dev)
        nv.aligner_scores(qd, kd, t_dev, n_dev, tau, lp, scores, ws, keep)
        if keep:
            ctx.tau = tau
            ctx.save_for_backward(qd, kd, t_dev, n_dev, ws)
        return scores

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        q, k, t_dev, n_dev, kept = ctx.saved_tensors
        B, T, C = q.shape
        N = k.shape[1]
        g = _dense_rows(grad.float())
        dq, dk = torch.empty_like(q), torch.empty_like(k)
        dlogp = torch.empty(B, T, N, dtype=torch.float32, device=q.device) if ctx.needs_input_grad[2] else None
        ws = torch.empty(nv.aligner_workspace(B, T, N, C, 2), dtype=torch.uint8, device=q.device)
        nv.aligner_scores_backward(q, k, t_dev, n_dev, ctx.tau, g, dq, dk, dlogp, kept, ws)
        return dq, dk, dlogp, None, None, None, None


def aligner_scores(queries, keys, t_lengths=None, n_lengths=None, temperature=0.0005, log_prior=None):
    """``scores`` (B, T, N) float32 of a learned aligner: s(t,n) = z(t,n) - log sum_{n'} exp z(t,n') + log_prior(t,n) with
    z(t,n) = -temperature |q_t - k_n|^2, the sum over the utterance's own tokens, -inf at and beyond an utterance's frames and
    tokens, so that ``exp(scores)`` without a prior is an attention map.  ``queries`` (B, T, C) or (T, C) and ``keys`` (B, N, C) or
    (N, C) are float32 device tensors, channel-last, 1 <= C <= 512, T <= 4096, N <= 1024 (more tokens than frames are allowed
    here; the path functions refuse them); ``log_prior`` is None or a float32 (B, T, N) device tensor, -inf allowed
    (``beta_binomial_log_prior``).  Differentiable once with respect to all three; exact zeros in the padding.  Under ``no_grad``,
    or where no input requires a gradient, nothing is kept."""
    who = "aligner_scores"
    for name, t in (("queries", queries), ("keys", keys)) + ((("log_prior", log_prior),) if log_prior is not None else ()):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise TypeError("%s: expected float32 %s, got %s" % (who, name, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if queries.dim() == 2 and keys.dim() == 2:
        queries, keys = queries.unsqueeze(0), keys.unsqueeze(0)
        if log_prior is not None and log_prior.dim() == 2:
            log_prior = log_prior.unsqueeze(0)
    if queries.dim() != 3 or keys.dim() != 3 or min(queries.shape) < 1 or min(keys.shape) < 1 \
            or queries.shape[0] != keys.shape[0] or queries.shape[2] != keys.shape[2]:
        raise ValueError("%s: expected queries (B, T, C) or (T, C) and keys (B, N, C) or (N, C), got shapes %s and %s"
                         % (who, tuple(queries.shape), tuple(keys.shape)))
    B, T, C = queries.shape
    N = keys.shape[1]
    if C > MAX_CHANNELS:
        raise ValueError("%s: %d channels exceed the limit of %d" % (who, C, MAX_CHANNELS))
    if log_prior is not None and tuple(log_prior.shape) != (B, T, N):
        raise ValueError("%s: expected a log_prior of shape (%d, %d, %d), got %s" % (who, B, T, N, tuple(log_prior.shape)))
    if not (isinstance(temperature, (int, float)) and 0.0 < float(temperature) < float("inf")):
        raise ValueError("%s: the temperature must be a positive number, got %r" % (who, temperature))
    tl, nl = _aligner_lengths(who, t_lengths, n_lengths, B, T, N)
    for name, t in (("queries", queries), ("keys", keys), ("log_prior", log_prior)):
        if t is not None:
            _require_device(t)
            if t.device != queries.device:
                raise ValueError("%s: queries are on %s and %s on %s" % (who, queries.device, name, t.device))
    keep = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (queries, keys, log_prior))
    return _AlignerScores.apply(queries, keys, log_prior, tl, nl, float(temperature), keep)


@torch.no_grad()
def beta_binomial_log_prior(t_lengths, n_lengths, scaling=1.0, T=None, N=None, device=None):
    """``log_prior`` (B, T, N) float32: for frame t of an utterance of T_b frames and N_b tokens the log of the beta-binomial
    distribution over the tokens n = 0 .. N_b - 1 with m = N_b - 1 trials, a = scaling (t + 1), b = scaling (T_b - t), evaluated
    in float64 and rounded once; every row sums to 1, one token gives 0, the padding holds -inf.  ``T`` / ``N`` default to the
    longest utterance's, ``device`` to the current one."""
    who = "beta_binomial_log_prior"
    tl = _lengths(t_lengths, len(t_lengths) if hasattr(t_lengths, "__len__") else 0, None, who + ": t_")
    nl = _lengths(n_lengths, len(tl), None, who + ": n_")
    if not tl:
        raise ValueError("%s: expected the frames and tokens of at least one utterance" % who)
    T, N = (max(tl) if T is None else int(T)), (max(nl) if N is None else int(N))
    tl, nl = _aligner_lengths(who, tl, nl, len(tl), T, N)
    if not (isinstance(scaling, (int, float)) and 0.0 < float(scaling) <= 1e6):
        raise ValueError("%s: the scaling must lie in (0, 1e6], got %r" % (who, scaling))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None and not nv.validate_only() else torch.device(device or "cpu")
    out = torch.empty(len(tl), T, N, dtype=torch.float32, device=dev)
    _require_device(out)
    t_dev, n_dev = (torch.tensor(v, dtype=torch.int32).to(dev) for v in (tl, nl))
    nv.beta_binomial_log_prior(t_dev, n_dev, float(scaling), out)
    return out


class AlignerScores(torch.nn.Module):
    """``aligner_scores`` at a fixed ``temperature``, with the beta-binomial prior of ``prior_scaling`` added where that is set.
    It holds no weights: the encoders that make queries and keys are the caller's."""

    def __init__(self, temperature=0.0005, prior_scaling=None):
        super().__init__()
        if not (isinstance(temperature, (int, float)) and 0.0 < float(temperature) < float("inf")):
            raise ValueError("AlignerScores: the temperature must be a positive number, got %r" % (temperature,))
        if prior_scaling is not None and not (isinstance(prior_scaling, (int, float)) and 0.0 < float(prior_scaling) <= 1e6):
            raise ValueError("AlignerScores: prior_scaling must be None or lie in (0, 1e6], got %r" % (prior_scaling,))
        self.temperature, self.prior_scaling = float(temperature), prior_scaling

    def forward(self, queries, keys, t_lengths=None, n_lengths=None):
        prior = None
        if self.prior_scaling is not None and torch.is_tensor(queries) and torch.is_tensor(keys) and queries.dim() == keys.dim() \
                and queries.dim() in (2, 3):
            B = 1 if queries.dim() == 2 else queries.shape[0]
            T, N = queries.shape[-2], keys.shape[-2]
            tl, nl = _aligner_lengths("aligner_scores", t_lengths, n_lengths, B, T, N)
            prior = beta_binomial_log_prior(tl, nl, self.prior_scaling, T, N, queries.device)
        return aligner_scores(queries, keys, t_lengths, n_lengths, self.temperature, prior)
