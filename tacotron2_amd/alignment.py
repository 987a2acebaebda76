"""Forced alignment on the GPU: the best monotonic path through a (frames, tokens) score matrix (csrc/align.hip, DESIGN.md
section 18; Glow-TTS's "monotonic alignment search"), per-token durations from a Tacotron 2 attention matrix, and what the
attention did beside that path; and the sum over all such paths (csrc/forward_sum.hip; the forward-sum
alignment likelihood of "One TTS Alignment To Rule Them All") with its gradient, the posterior occupancy of every cell; and the
scores a learned aligner feeds both with (csrc/aligner.hip, csrc/aligner_rows.hip): the distances between
projected frames and projected tokens, normalised over the tokens, plus a beta-binomial prior, with their gradient; and what
consumes a duration (csrc/regulate.hip): the length regulator of FastSpeech and FastPitch, which repeats
token n's vector d(n) times, and the mean of a frame-rate quantity over each token's frames, both with their gradients.

    durations, score = monotonic_align(scores, t_lengths, n_lengths)
    durations, score, path = attention_durations(alignments, input_lengths, output_lengths, return_path=True)
    metrics = alignment_metrics(alignments, path, input_lengths, output_lengths)
    log_z = forward_sum(scores, t_lengths, n_lengths)                      # differentiable: d log_z / d scores = gamma
    gamma, soft_durations, log_z = alignment_posterior(scores, t_lengths, n_lengths)
    loss = ForwardSumLoss(reduction='mean', per_frame=False)(scores, t_lengths, n_lengths)
    scores = aligner_scores(queries, keys, t_lengths, n_lengths, temperature=0.0005, log_prior=None)   # differentiable
    log_prior = beta_binomial_log_prior(t_lengths, n_lengths, scaling=1.0)
    scores = AlignerScores(temperature=0.0005, prior_scaling=1.0)(queries, keys, t_lengths, n_lengths)
    path, t_lengths = durations_to_path(durations, n_lengths, T=None)
    y, t_lengths = length_regulate(x, durations, n_lengths, T=None)         # differentiable in x
    y, t_lengths = LengthRegulator(pace=1.0, rounding=True, max_len=None)(x, durations, n_lengths)
    per_token = token_average(values, durations, n_lengths, weights=None)   # differentiable in values

``monotonic_align``, ``attention_durations``, ``alignment_metrics``, ``beta_binomial_log_prior`` and ``durations_to_path`` have no
gradient; ``forward_sum``, ``ForwardSumLoss``, ``aligner_scores``, ``AlignerScores``, ``length_regulate``, ``LengthRegulator`` and
``token_average`` have one.  There is no CPU path."""
import numpy as np
import torch

from . import native as nv
from . import ragged as rg
from .audio import _lengths
from .ragged import dense_rows as _dense_rows, require_device as _require_device

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
    scores, tl, nl = _path_args("monotonic_align", scores, t_lengths, n_lengths)
    B, T, N = scores.shape
    s, t_dev, n_dev = _longest_part(scores, tl, nl)
    Tm, Nm = s.shape[1:]
    dev = scores.device
    durations = torch.empty(B, Nm, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    path = torch.empty(B, Tm, dtype=torch.int32, device=dev) if return_path else None
    nv.monotonic_align(s, t_dev, n_dev, durations, score, path, rg.workspace(nv.align_workspace(B, Tm, Nm), dev))
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


def _path_args(who, scores, t_lengths, n_lengths):
    """What ``monotonic_align`` and the forward-sum functions ask of their arguments -> (scores as (B, T, N), frames, tokens)."""
    rg.float32(who, scores)
    if scores.dim() == 2:
        scores = scores.unsqueeze(0)
    if scores.dim() != 3 or min(scores.shape) < 1:
        raise ValueError("%s: expected (B, T, N) or (T, N) scores, got shape %s" % (who, tuple(scores.shape)))
    _require_device(scores)
    B, T, N = scores.shape
    return (scores,) + rg.path_lengths(who, t_lengths, n_lengths, B, T, N, (MAX_FRAMES, MAX_TOKENS), monotonic=True)


def _longest_part(scores, tl, nl):
    """The longest utterance's part of ``scores`` with unit stride along N, and the lengths on its device."""
    s = scores.detach()[:, :max(tl), :max(nl)]
    if s.shape[2] > 1 and s.stride(2) != 1:
        s = s.contiguous()
    return (s,) + rg.upload(scores.device, tl, nl)


def _forward_sum_launch(scores, tl, nl, keep):
    """The alpha launch over the longest utterance's part of ``scores`` -> (that part, device lengths, log_z, workspace)."""
    s, t_dev, n_dev = _longest_part(scores, tl, nl)
    B, Tm, Nm = s.shape
    log_z = torch.empty(B, dtype=torch.float32, device=s.device)
    ws = rg.workspace(nv.forward_sum_workspace(B, Tm, Nm, keep), s.device)
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
    scores, tl, nl = _path_args("forward_sum", scores, t_lengths, n_lengths)
    return _ForwardSum.apply(scores, tl, nl, torch.is_grad_enabled() and scores.requires_grad)


@torch.no_grad()
def alignment_posterior(scores, t_lengths=None, n_lengths=None):
    """-> ``gamma`` (B, T, N) float32, the posterior probability that a path drawn in proportion to exp(its score) is on token n
    at frame t (d log_z / d scores; a row within an utterance sums to 1, zeros in the padding), ``soft_durations`` (B, N) float32,
    its column sums (the expected frames on each token; a row sums to the utterance's T), and ``log_z`` (B,) as ``forward_sum``
    gives it.  An utterance without a possible path has zeros and -inf."""
    scores, tl, nl = _path_args("forward_sum", scores, t_lengths, n_lengths)
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
        scores, tl, nl = _path_args("forward_sum", scores, t_lengths, n_lengths)
        loss = -forward_sum(scores, tl, nl)
        if self.per_frame:
            loss = loss / torch.tensor(tl, dtype=torch.float32).to(loss.device)
        return loss if self.reduction == 'none' else loss.mean() if self.reduction == 'mean' else loss.sum()


def _aligner_lengths(who, t_lengths, n_lengths, B, T, N):
    return rg.path_lengths(who, t_lengths, n_lengths, B, T, N, (MAX_FRAMES, MAX_TOKENS))


class _AlignerScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, logp, tl, nl, tau, keep):
        B, T, C = q.shape
        N = k.shape[1]
        dev = q.device
        qd, kd = q.detach().contiguous(), k.detach().contiguous()
        lp = None if logp is None else _dense_rows(logp.detach())
        t_dev, n_dev = rg.upload(dev, tl, nl)
        scores = torch.empty(B, T, N, dtype=torch.float32, device=dev)
        ws = rg.workspace(nv.aligner_workspace(B, T, N, C, 1 if keep else 0), dev)
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
        ws = rg.workspace(nv.aligner_workspace(B, T, N, C, 2), q.device)
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
        rg.float32(who, t, name)
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
    tau = rg.positive(who, temperature, "the temperature must be a positive number")
    tl, nl = _aligner_lengths(who, t_lengths, n_lengths, B, T, N)
    for name, t in (("queries", queries), ("keys", keys), ("log_prior", log_prior)):
        if t is not None:
            _require_device(t)
            if t.device != queries.device:
                raise ValueError("%s: queries are on %s and %s on %s" % (who, queries.device, name, t.device))
    keep = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (queries, keys, log_prior))
    return _AlignerScores.apply(queries, keys, log_prior, tl, nl, tau, keep)


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
    scaling = rg.positive(who, scaling, "the scaling must lie in (0, 1e6]", cap=1e6)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None and not nv.validate_only() else torch.device(device or "cpu")
    out = torch.empty(len(tl), T, N, dtype=torch.float32, device=dev)
    _require_device(out)
    nv.beta_binomial_log_prior(*rg.upload(dev, tl, nl), scaling, out)
    return out


class AlignerScores(torch.nn.Module):
    """``aligner_scores`` at a fixed ``temperature``, with the beta-binomial prior of ``prior_scaling`` added where that is set.
    It holds no weights: the encoders that make queries and keys are the caller's."""

    def __init__(self, temperature=0.0005, prior_scaling=None):
        super().__init__()
        self.temperature = rg.positive("AlignerScores", temperature, "the temperature must be a positive number")
        if prior_scaling is not None:
            rg.positive("AlignerScores", prior_scaling, "prior_scaling must be None or lie in (0, 1e6]", cap=1e6)
        self.prior_scaling = prior_scaling

    def forward(self, queries, keys, t_lengths=None, n_lengths=None):
        prior = None
        if self.prior_scaling is not None and torch.is_tensor(queries) and torch.is_tensor(keys) and queries.dim() == keys.dim() \
                and queries.dim() in (2, 3):
            B = 1 if queries.dim() == 2 else queries.shape[0]
            T, N = queries.shape[-2], keys.shape[-2]
            tl, nl = _aligner_lengths("aligner_scores", t_lengths, n_lengths, B, T, N)
            prior = beta_binomial_log_prior(tl, nl, self.prior_scaling, T, N, queries.device)
        return aligner_scores(queries, keys, t_lengths, n_lengths, self.temperature, prior)


# ---- the length regulator (csrc/regulate.hip) ----------------------------------------------------------------
MAX_REGULATED_FRAMES = 65536


def _regulate_args(who, durations, n_lengths, batch_of_one):
    """``durations`` as (B, N) int32 or int64 with unit stride along N, and the token counts as a device int32 vector or None.
    Token counts given on the host are checked against [0, N]; a device tensor is not read here, the kernel clamps it."""
    if not torch.is_tensor(durations) or durations.dtype not in (torch.int32, torch.int64):
        raise TypeError("%s: expected int32 or int64 durations, got %s"
                        % (who, durations.dtype if torch.is_tensor(durations) else type(durations).__name__))
    if batch_of_one and durations.dim() == 1:
        durations = durations.unsqueeze(0)
    if durations.dim() != 2 or min(durations.shape) < 1:
        raise ValueError("%s: expected (B, N) or (N,) durations with at least one token, got shape %s" % (who, tuple(durations.shape)))
    _require_device(durations)
    B, N = durations.shape
    if N > MAX_TOKENS:
        raise ValueError("%s: %d tokens exceed the limit of %d" % (who, N, MAX_TOKENS))
    durations = durations.detach()
    if N > 1 and durations.stride(1) != 1 or (B > 1 and durations.stride(0) < N):
        durations = durations.contiguous()
    return durations, rg.device_lengths(who, n_lengths, B, N, durations.device, "durations are", rg.TOKENS)


def _regulate_frames(who, durations, n_dev, T):
    """The output's frame count: ``T`` itself, or with None the largest sum of the batch, by the call's one device-to-host read,
    which also brings the sign check."""
    if T is not None:
        if isinstance(T, bool) or not isinstance(T, int) or not 0 <= T <= MAX_REGULATED_FRAMES:
            raise ValueError("%s: T must be None or an int in [0, %d], got %r" % (who, MAX_REGULATED_FRAMES, T))
        return T
    B = durations.shape[0]
    totals = torch.empty(B, dtype=torch.int64, device=durations.device)
    nv.durations_to_path(durations, n_dev, 0, None, torch.empty(B, dtype=torch.int32, device=durations.device), None, totals)
    lo, hi = torch.stack((totals.min(), totals.max())).tolist()             # the one read
    if lo < 0:
        raise ValueError("%s: negative durations" % who)
    if hi > MAX_REGULATED_FRAMES:
        raise ValueError("%s: durations sum to %d frames, more than the limit of %d; name T to cut them" % (who, hi, MAX_REGULATED_FRAMES))
    return int(hi)


def _paths(durations, n_dev, T, want_path, want_ends):
    B, N = durations.shape
    dev = durations.device
    t_lengths = torch.empty(B, dtype=torch.int32, device=dev)
    path = torch.empty(B, T, dtype=torch.int32, device=dev) if want_path else None
    ends = torch.empty(B, N, dtype=torch.int32, device=dev) if want_ends else None
    nv.durations_to_path(durations, n_dev, T, path, t_lengths, ends)
    return path, t_lengths, ends


@torch.no_grad()
def durations_to_path(durations, n_lengths=None, T=None):
    """The token of every frame under the int32 or int64 device tensor ``durations`` (B, N) or (N,), d >= 0: with e(n) = d(0) + ..
    + d(n) over the utterance's ``n_lengths`` tokens (0 <= N_b <= N; all N where None; what lies beyond is ignored) and
    T_b = min(e(N_b - 1), T), path(t) is the smallest n with e(n) > t for t < T_b and -1 from T_b on; a token of duration 0 owns no
    frame.  -> ``path`` (B, T) int32 and ``t_lengths`` (B,) int32 = T_b.  For the durations ``monotonic_align`` returns this is the
    path it returns.

    With ``T=None`` the frame count is the largest sum of the batch, found by one device-to-host read (a synchronisation); the
    same read refuses negative durations and sums above 65 536.  With ``T`` an int nothing is read back and the call does not
    synchronise: longer utterances are cut at T, and an utterance with a negative duration is marked on the device instead of
    refused: its ``t_lengths`` entry is -1 and it has no frames.  N <= 1024, T <= 65 536."""
    who = "durations_to_path"
    d, n_dev = _regulate_args(who, durations, n_lengths, True)
    T = _regulate_frames(who, d, n_dev, T)
    path, t_lengths, _ = _paths(d, n_dev, T, True, False)
    return path, t_lengths


class _LengthRegulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, durations, n_dev, T, keep):
        B, N, C = x.shape
        path, t_lengths, ends = _paths(durations, n_dev, T, T > 0, keep)
        y = torch.empty(B, T, C, dtype=torch.float32, device=x.device)
        if T > 0:
            nv.length_regulate(_dense_rows(x.detach()), path, y)
        if keep:
            ctx.save_for_backward(ends)
        ctx.mark_non_differentiable(t_lengths)
        return y, t_lengths

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad, _):
        ends, = ctx.saved_tensors
        B, T, C = grad.shape
        if T == 0:
            return torch.zeros(B, ends.shape[1], C, dtype=torch.float32, device=grad.device), None, None, None, None
        dx = torch.empty(B, ends.shape[1], C, dtype=torch.float32, device=grad.device)
        nv.length_regulate_backward(_dense_rows(grad.float()), ends, dx)   # an expanded gradient is copied
        return dx, None, None, None, None


def length_regulate(x, durations, n_lengths=None, T=None):
    """The length regulator: token n's vector repeated d(n) times.  ``x`` is a float32 device tensor (B, N, C) or (N, C) (a batch
    of one, with (N,) durations), 1 <= C <= 512; ``durations``, ``n_lengths`` and ``T`` are those of ``durations_to_path``.
    -> ``y`` (B, T, C) float32 with y(t, :) = x(path(t), :) below the utterance's T_b and +0 from there on, and ``t_lengths`` (B,)
    int32 = T_b.  It is a copy: every finite value, infinity, NaN and -0 keeps its bits.  Differentiable once with respect to
    ``x``: dx(n, :) is the sum of dy(t, :) over the token's frames, t ascending, in plain float32 adds; +0 for a token without a
    frame and at and beyond N_b; frames cut off by T contribute nothing.

    With ``T=None`` the frame count is the largest sum of the batch, found by one device-to-host read (a synchronisation), which
    also refuses negative durations; an all-zero batch gives T = 0 and an empty ``y``.  With ``T`` an int there is no
    synchronisation anywhere in the call; an utterance with a negative duration then has ``t_lengths`` = -1 and a ``y`` of
    zeros.  A non-contiguous ``x`` or gradient is made contiguous."""
    who = "length_regulate"
    rg.float32(who, x)
    if x.dim() == 2 and torch.is_tensor(durations) and durations.dim() == 1:
        x, durations = x.unsqueeze(0), durations.unsqueeze(0)
    if x.dim() != 3 or min(x.shape) < 1:
        raise ValueError("%s: expected (B, N, C) or (N, C) tokens, got shape %s" % (who, tuple(x.shape)))
    _require_device(x)
    if torch.is_tensor(durations) and durations.device != x.device:
        raise ValueError("%s: the tokens are on %s and the durations on %s" % (who, x.device, durations.device))
    d, n_dev = _regulate_args(who, durations, n_lengths, False)
    if tuple(d.shape) != tuple(x.shape[:2]):
        raise ValueError("%s: expected durations of shape %s, got %s" % (who, tuple(x.shape[:2]), tuple(d.shape)))
    if x.shape[2] > MAX_CHANNELS:
        raise ValueError("%s: %d channels exceed the limit of %d" % (who, x.shape[2], MAX_CHANNELS))
    T = _regulate_frames(who, d, n_dev, T)
    return _LengthRegulate.apply(x, d, n_dev, T, torch.is_grad_enabled() and x.requires_grad)


class LengthRegulator(torch.nn.Module):
    """``length_regulate`` with the frame count ``max_len`` (None: the batch's longest, one synchronisation).  Integer durations
    pass through; float durations (a duration predictor's output at inference) become d = max(0, round(durations / pace)), or the
    floor instead of the rounding where ``rounding`` is False, in one elementwise pass.  It holds no weights."""

    def __init__(self, pace=1.0, rounding=True, max_len=None):
        super().__init__()
        pace = rg.positive("LengthRegulator", pace, "the pace must be a positive number")
        if max_len is not None and (isinstance(max_len, bool) or not isinstance(max_len, int) or not 0 <= max_len <= MAX_REGULATED_FRAMES):
            raise ValueError("LengthRegulator: max_len must be None or an int in [0, %d], got %r" % (MAX_REGULATED_FRAMES, max_len))
        self.pace, self.rounding, self.max_len = pace, bool(rounding), max_len

    def forward(self, x, durations, n_lengths=None):
        if torch.is_tensor(durations) and durations.is_floating_point():
            d = durations.detach() / self.pace
            durations = (torch.round(d) if self.rounding else torch.floor(d)).clamp_(0, 2147483647).to(torch.int32)
        return length_regulate(x, durations, n_lengths, self.max_len)


class _TokenAverage(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, durations, n_dev, w, keep):
        B, T, C = v.shape
        N = durations.shape[1]
        path, _, ends = _paths(durations, n_dev, T, keep, True)
        vd = _dense_rows(v.detach())
        mean = torch.empty(B, N, C, dtype=torch.float32, device=v.device)
        den = torch.empty(B, N, dtype=torch.float32, device=v.device)
        nv.token_average(vd, w, ends, mean, den)
        if keep:
            ctx.save_for_backward(path, den, w)
        return mean

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        path, den, w = ctx.saved_tensors
        dv = torch.empty(grad.shape[0], path.shape[1], grad.shape[2], dtype=torch.float32, device=grad.device)
        nv.token_average_backward(grad.float().contiguous(), den, w, path, dv)
        return dv, None, None, None, None


def token_average(values, durations, n_lengths=None, weights=None):
    """The mean of a frame-rate quantity over each token's frames.  ``values`` is a float32 device tensor (B, T) or (B, T, C),
    1 <= C <= 512, T <= 65 536; its T is the frame count (durations that sum past it are cut there, as in ``durations_to_path``
    with that T); ``durations`` (B, N) and ``n_lengths`` are those of ``durations_to_path``; ``weights`` is None (ones) or a
    non-negative float32 device tensor (B, T).  With the token's frames t ascending, num = fmaf(w(t), v(t), num) and
    den = den + w(t), both from +0, and the result is num / den where den > 0 and +0 elsewhere: a token without frames, or whose
    frames all weigh 0 (the mean over the voiced frames, with the voiced flags as weights).  -> (B, N) or (B, N, C) float32.
    Differentiable once with respect to ``values``: dv(t) = w(t) * (g(path(t)) / den(path(t))), +0 where den = 0 and beyond the
    utterance's frames; ``weights`` gets no gradient.  The call never synchronises: an utterance with a negative duration is not
    refused, it gives zeros."""
    who = "token_average"
    rg.float32(who, values, "values")
    if values.dim() not in (2, 3) or min(values.shape) < 1:
        raise ValueError("%s: expected (B, T) or (B, T, C) values, got shape %s" % (who, tuple(values.shape)))
    flat = values.dim() == 2
    v = values.unsqueeze(2) if flat else values
    B, T, C = v.shape
    _require_device(v)
    if T > MAX_REGULATED_FRAMES or C > MAX_CHANNELS:
        raise ValueError("%s: %d frames and %d channels exceed the limits of %d frames and %d channels"
                         % (who, T, C, MAX_REGULATED_FRAMES, MAX_CHANNELS))
    if torch.is_tensor(durations) and durations.device != v.device:
        raise ValueError("%s: the values are on %s and the durations on %s" % (who, v.device, durations.device))
    d, n_dev = _regulate_args(who, durations, n_lengths, False)
    if d.shape[0] != B:
        raise ValueError("%s: expected durations (%d, N), got shape %s" % (who, B, tuple(d.shape)))
    w = None
    if weights is not None:
        rg.float32(who, weights, "weights")
        if tuple(weights.shape) != (B, T):
            raise ValueError("%s: expected weights of shape (%d, %d), got %s" % (who, B, T, tuple(weights.shape)))
        if weights.device != v.device:
            raise ValueError("%s: the values are on %s and the weights on %s" % (who, v.device, weights.device))
        w = weights.detach()
        if (T > 1 and w.stride(1) != 1) or (B > 1 and w.stride(0) < T):
            w = w.contiguous()
    mean = _TokenAverage.apply(v, d, n_dev, w, torch.is_grad_enabled() and values.requires_grad)
    return mean.squeeze(2) if flat else mean
