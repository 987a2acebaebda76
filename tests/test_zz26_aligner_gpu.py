"""The learned-aligner scores on the MI355X (alignment.aligner_scores, alignment.beta_binomial_log_prior, alignment.AlignerScores,
csrc/aligner.hip, csrc/aligner_rows.hip, tools/bench_aligner.py) against the float64 restatement (tests/aligner_ref.py).

Per case and per tensor (the scores, the kept lse, dQ, dK) the largest absolute error over the utterance's region is at most
max(4 x the float32 restatement's own largest error on that case, 8 2^-24 max(1, largest |value| of that tensor in float64))
(DESIGN.md section 20.4); the prior is held to 4 2^-24 max(1, |logp|) per element.  Every case prints its ratios error / allowed
(``FIGURE`` lines; profiles/aligner_pytest_gpu.txt has the run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import align_ref
import aligner_cases as ac
import aligner_ref as ar
import forward_sum_cases as fc
import forward_sum_ref as fr
import golden_util as gu
from test_forward_sum_cpu import ctc_neg_log_z

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("prior", (False, True))
@pytest.mark.parametrize("tau", ac.TAUS)
@pytest.mark.parametrize("which", range(len(ac.SHAPES)))
def test_shapes(native_lib, which, tau, prior):
    """The scores, lse, dQ, dK and dlogp for a random g, then for g = -gamma of the forward-sum posterior of the device's scores."""
    from tacotron2_amd import alignment
    T, N, C = ac.SHAPES[which]
    c = ac.case(T, N, C, tau, prior)
    out = ac.run([c], DEV, offset=(T + N) % 3)
    ac.check_case(c, out, label="random g ")
    s = torch.from_numpy(out["s"]).to(DEV)
    gamma, _, log_z = alignment.alignment_posterior(s)
    best = alignment.monotonic_align(s)[1]
    x = out["s"][0]
    tz, _, _ = fc.allowed(fr.forward_sum32(x), fr.forward_sum64(x))
    assert float(best[0]) <= float(log_z[0]) + tz + align_ref.bound(T, abs(float(best[0]))), (T, N, float(best[0]), float(log_z[0]))
    g = (-gamma[0]).cpu().numpy()
    ac.check_case(c, ac.run([c], DEV, offset=1, grads=[g]), g=g, label="g = -gamma ")


def test_ragged_batch_equals_each_utterance_alone_and_two_calls_agree(native_lib):
    ac.ragged_equals_alone(DEV)


def test_more_utterances_than_compute_units(native_lib):
    ac.many_short(DEV)


def test_a_column_of_minus_infinity_in_the_prior(native_lib):
    ac.ninf_column(DEV)


def test_row_kernels_alone(native_lib):
    for T, N in ac.ROW_SHAPES:
        mat = ac.row_mat(T, N)
        ac.check_rows(mat, ac.run_rows([mat], DEV, offset=(T + N) % 3))


def test_prior(native_lib):
    from tacotron2_amd import alignment
    for scaling in (1.0, 0.25):
        ac.check_prior(DEV, [(12, 8), (5, 1), (1, 1), (130, 65), (870, 187), (40, 90)], scaling, alignment.beta_binomial_log_prior)
    ac.check_prior(DEV, [(4095, 1022)], 1.0, alignment.beta_binomial_log_prior)     # a buffer of 4096 x 1024, both limits


def test_module_equals_the_native_calls_and_autograd(native_lib):
    from tacotron2_amd import alignment
    cases = ac.ragged_cases(0.5)
    out = ac.run(cases, DEV)
    B, C = len(cases), 80
    tl, nl = [c["T"] for c in cases], [c["N"] for c in cases]
    q, k, lp = torch.zeros(B, max(tl), C), torch.zeros(B, max(nl), C), torch.zeros(B, max(tl), max(nl))
    g = torch.zeros(B, max(tl), max(nl))
    for b, c in enumerate(cases):
        q[b, :tl[b]], k[b, :nl[b]], g[b, :tl[b], :nl[b]] = (torch.from_numpy(np.array(c[n])) for n in ("q", "k", "g"))
        if c["logp"] is not None:
            lp[b, :tl[b], :nl[b]] = torch.from_numpy(np.array(c["logp"]))
    q, k, lp, g = (t.to(DEV) for t in (q, k, lp, g))
    plain = alignment.aligner_scores(q, k, tl, nl, 0.5, lp)
    assert plain.grad_fn is None and np.array_equal(ac.bits(plain.cpu().numpy()), ac.bits(out["s"]))
    leaves = [t.clone().requires_grad_(True) for t in (q, k, lp)]
    s = alignment.aligner_scores(leaves[0], leaves[1], torch.tensor(tl), torch.tensor(nl), 0.5, leaves[2])
    assert s.grad_fn is not None and torch.equal(s.detach(), plain)
    with torch.no_grad():
        assert alignment.aligner_scores(leaves[0], leaves[1], tl, nl, 0.5, leaves[2]).grad_fn is None
    torch.where(torch.isfinite(s), s * g, torch.zeros_like(s)).sum().backward()
    for leaf, name in zip(leaves, ("dq", "dk", "dlogp")):
        assert np.array_equal(ac.bits(leaf.grad.cpu().numpy()), ac.bits(out[name])), name
    # a non-contiguous input is made contiguous; (T, C) and (N, C) are a batch of one; only the keys need a gradient
    qt = q[0, :tl[0]].t().contiguous().t()
    k1 = k[0, :nl[0]].clone().requires_grad_(True)
    one = alignment.aligner_scores(qt, k1, temperature=0.5, log_prior=lp[0, :tl[0], :nl[0]])
    assert not qt.is_contiguous() and tuple(one.shape) == (1, tl[0], nl[0])
    assert np.array_equal(ac.bits(one.detach().cpu().numpy()[0]), ac.bits(out["s"][0, :tl[0], :nl[0]]))
    (one * g[:1, :tl[0], :nl[0]]).sum().backward()
    assert np.array_equal(ac.bits(k1.grad.cpu().numpy()), ac.bits(out["dk"][0, :nl[0]]))
    # the module: no prior, and the beta-binomial prior built inside
    mod = alignment.AlignerScores(0.5)
    assert not list(mod.parameters()) and torch.equal(mod(q, k, tl, nl), alignment.aligner_scores(q, k, tl, nl, 0.5))
    with_prior = alignment.AlignerScores(0.5, prior_scaling=1.0)(q, k, tl, nl)
    want = alignment.aligner_scores(q, k, tl, nl, 0.5, alignment.beta_binomial_log_prior(tl, nl, 1.0, max(tl), max(nl)))
    assert torch.equal(with_prior, want)
    from tacotron2_amd import native
    with pytest.raises(native.NativeError, match="no CPU path"):
        alignment.aligner_scores(q.cpu(), k.cpu())


def test_no_grad_allocates_no_slab(native_lib):
    """The caching allocator hands out blocks up to 1 MiB larger than asked for and rounds to 2 MiB, so the shape makes the
    forward's workspace (the key slab, 33 MB) many times that slack and the output small beside it."""
    from tacotron2_amd import alignment, native
    B, T, N, C = 16, 64, 1024, 512
    q, k = torch.randn(B, T, C, device=DEV), torch.randn(B, N, C, device=DEV)
    alignment.aligner_scores(q, k)                                          # the allocator's pools are warm
    torch.cuda.synchronize()
    small, kept = native.aligner_workspace(B, T, N, C, 0), native.aligner_workspace(B, T, N, C, 1)
    out_bytes, slack = 4 * B * T * N, 4 << 20
    assert kept == small + 4 * B * T and small == 4 * B * N * C + 4 * B * N and small > 8 * slack
    for leaf, keeps in ((q, False), (q.clone().requires_grad_(True), True)):
        for grad_mode in (False, True):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            with torch.set_grad_enabled(grad_mode):
                out = alignment.aligner_scores(leaf, k)
            torch.cuda.synchronize()
            peak, after = torch.cuda.max_memory_allocated() - before, torch.cuda.memory_allocated() - before
            assert small <= peak < out_bytes + kept + 2 * slack, (keeps, grad_mode, peak)
            if keeps and grad_mode:
                assert out.grad_fn is not None and after >= out_bytes + kept
            else:                                                           # the output alone: the workspace is gone
                assert out.grad_fn is None and after < out_bytes + slack, (keeps, grad_mode, peak, after)
            del out


def test_forward_sum_loss_of_the_scores_against_float64_autograd(native_lib):
    """ForwardSumLoss('sum')(aligner_scores(q, k, log_prior=p)) and both gradients.

    1. The composed gradients are, bit for bit, the native backward fed g = -gamma of ``alignment_posterior`` on the device's own
       scores, and with that gamma handed to both restatements as data they meet the convention of section 20.4.
    2. End to end against float64 torch autograd through the restated scores and ``F.ctc_loss`` with a blank of -inf.  The
       gradient ``F.ctc_loss`` returns is exp(lp) - gamma, that with respect to the logits of a log_softmax, which equals -gamma
       behind one only where the rows of exp(lp) sum to 1; with a prior added they do not, so the reference subtracts
       (exp(s).detach() s).sum(), whose gradient takes the exp(lp) out again (held to ``grads64`` of the float64 gamma here).
       The loss is held to the case's log Z tolerance tz (section 19.4) plus T ts, ts the scores' allowed error (log Z moves by at
       most the sum of the score errors along a path).  For the gradients: the device's gamma differs from the float64 one by at
       most e_g(t,n) = tg + 2 T ts gamma(t,n): tg is section 19.4's tolerance of gamma, and a perturbation of every score by at
       most ts moves gamma(t,n) by at most ts sum_{t',n'} |Cov(on (t,n), on (t',n'))| <= 2 T ts gamma(t,n).  With dz = -gamma + p
       (G = -1) and p within 2 ts p, |d dz(t,n)| <= E(t,n) = e_g(t,n) + p(t,n) sum_n' e_g(t,n') + 2 ts p(t,n), so element by
       element |d dQ| <= 2 tau E |k| and |d dK(n,c)| <= 2 tau sum_t E(t,n) |q(t,c) - k(n,c)|, on top of the allowed error of the
       backward at the float64 gamma.  The largest allowance must stay below half the largest gradient: zeros cannot pass."""
    from tacotron2_amd import alignment
    for T, N, C, tau in ((65, 64, 80, 0.0005), (130, 63, 32, 1.0), (296, 257, 80, 0.05)):
        c = ac.case(T, N, C, tau, True, 7)
        q, k, lp = (torch.from_numpy(np.array(c[n])) for n in ("q", "k", "logp"))
        leaves = [t.to(DEV).requires_grad_(True) for t in (q, k)]
        s = alignment.aligner_scores(leaves[0], leaves[1], temperature=tau, log_prior=lp.to(DEV))
        loss = alignment.ForwardSumLoss('sum')(s)
        loss.backward()
        got_q, got_k = leaves[0].grad.cpu().numpy(), leaves[1].grad.cpu().numpy()
        # 1. the device's gamma as data
        g = (-alignment.alignment_posterior(s.detach())[0][0]).cpu().numpy()
        out = ac.run([c], DEV, grads=[g])
        assert np.array_equal(ac.bits(out["dq"][0]), ac.bits(got_q)) and np.array_equal(ac.bits(out["dk"][0]), ac.bits(got_k))
        ac.check_case(c, out, g=g, label="composed, g = -gamma ")
        # 2. float64 autograd end to end
        q64, k64 = q.double().requires_grad_(True), k.double().requires_grad_(True)
        z = -tau * ((q64[:, None, :] - k64[None, :, :]) ** 2).sum(dim=2)
        s64 = torch.log_softmax(z, dim=1) + lp.double()
        want = torch.nn.functional.ctc_loss(torch.cat([torch.full((T, 1), -np.inf, dtype=torch.float64), s64], dim=1).unsqueeze(1),
                                            torch.arange(1, N + 1).unsqueeze(0), torch.tensor([T]), torch.tensor([N]), blank=0,
                                            reduction='sum')
        (want - (torch.exp(s64).detach() * s64).sum()).backward()
        x = s64.detach().float().numpy()
        assert abs(float(ctc_neg_log_z(x)[0]) + fr.forward_sum64(x)[0]) <= 1e-9 * T
        tz, tg, _ = fc.allowed(fr.forward_sum32(x), fr.forward_sum64(x))
        ts = ar.allowed(c["f32"]["s"], c["f64"]["s"])
        gam = fr.forward_sum64(x)[1]
        own, ref = ar.grads32(c["q"], c["k"], tau, (-gam).astype(np.float32)), ar.grads64(c["q"], c["k"], tau, -gam)
        rq, rk = q64.grad.numpy(), k64.grad.numpy()
        assert np.abs(rq - ref[0]).max() <= 1e-5 * np.abs(rq).max() and np.abs(rk - ref[1]).max() <= 1e-5 * np.abs(rk).max()
        p = c["f64"]["p"]
        e_g = tg + 2 * T * ts * gam
        E = e_g + p * e_g.sum(axis=1, keepdims=True) + 2 * ts * p
        kd, qd = c["k"].astype(np.float64), c["q"].astype(np.float64)
        b_dq = ar.allowed(own[0], ref[0]) + 2 * tau * (E @ np.abs(kd))
        b_dk = ar.allowed(own[1], ref[1]) + 2 * tau * np.einsum('tn,tnc->nc', E, np.abs(qd[:, None, :] - kd[None, :, :]))
        b_loss = tz + T * ts
        e_loss = abs(float(loss.detach()) - float(want.detach()))
        e_dq, e_dk = np.abs(got_q - rq), np.abs(got_k - rk)
        print("FIGURE loss behind the scores (%d, %d, %d) tau %g: loss error %.3g (allowed %.3g); dQ error %.3g, allowed at most %.3g, "
              "worst error / allowed %.4f, largest |dQ| %.3g; dK error %.3g, allowed at most %.3g, worst error / allowed %.4f, "
              "largest |dK| %.3g" % (T, N, C, tau, e_loss, b_loss, e_dq.max(), b_dq.max(), (e_dq / b_dq).max(), np.abs(rq).max(),
                                     e_dk.max(), b_dk.max(), (e_dk / b_dk).max(), np.abs(rk).max()))
        assert e_loss <= b_loss and (e_dq <= b_dq).all() and (e_dk <= b_dk).all(), (T, N, C)
        assert b_dq.max() < 0.5 * np.abs(rq).max() and b_dk.max() < 0.5 * np.abs(rk).max(), (T, N, C)


def test_one_token_and_expanded_operands_through_autograd(native_lib):
    """N = 1: every score is 0 + log_prior and every gradient of q and k is 0; ``.sum().backward()`` hands over a gradient of
    stride (0, 0, 0), and an expanded log_prior has such strides too: both are copied, not refused."""
    from tacotron2_amd import alignment
    for B, T, C in ((1, 3, 2), (2, 5, 7)):
        q, k = (torch.randn(B, n, C, device=DEV).requires_grad_(True) for n in (T, 1))
        s = alignment.aligner_scores(q, k)
        assert tuple(s.shape) == (B, T, 1) and not s.detach().cpu().numpy().any()
        s.sum().backward()
        assert not q.grad.cpu().numpy().any() and not k.grad.cpu().numpy().any()
        lp = torch.full((1, 1, 1), -2.5, device=DEV).expand(B, T, 1).requires_grad_(True)
        s = alignment.aligner_scores(q, k, log_prior=lp)
        assert (s.detach().cpu().numpy() == np.float32(-2.5)).all()
        (3.0 * s).sum().backward()
    # the same kinds of strides at N > 1: an expanded gradient and a prior expanded over the batch
    c = ac.case(7, 7, 80, 1.0, True)
    q, k, lp = (torch.from_numpy(np.array(c[n])).to(DEV) for n in ("q", "k", "logp"))
    ql, kl = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    s = alignment.aligner_scores(torch.stack([ql, ql]), torch.stack([kl, kl]), temperature=1.0, log_prior=lp.unsqueeze(0).expand(2, 7, 7))
    s.sum().backward()
    out = ac.run([c], DEV, grads=[np.ones((7, 7), np.float32)])
    assert np.array_equal(ac.bits(s.detach().cpu().numpy()[1]), ac.bits(out["s"][0]))
    assert np.allclose(ql.grad.cpu().numpy(), 2 * out["dq"][0], rtol=1e-6, atol=1e-7)


def test_sliced_operands_at_any_alignment(native_lib):
    """A contiguous slice of a batch, or of a flat buffer, starts wherever it starts: C odd, and C a multiple of 4 one float off
    a 16-byte boundary, give the bits of an aligned copy."""
    from tacotron2_amd import alignment
    for C, off in ((5, 0), (80, 1), (80, 2), (33, 3)):
        g = torch.Generator().manual_seed(C + off)
        Q, K = torch.randn(3, 7, C, generator=g).to(DEV), torch.randn(3, 3, C, generator=g).to(DEV)
        flat_q, flat_k = torch.zeros(off + 7 * C + 8, device=DEV), torch.zeros(off + 3 * C + 8, device=DEV)
        for b in range(3):
            fq, fk = flat_q[off:off + 7 * C].view(7, C), flat_k[off:off + 3 * C].view(3, C)
            fq.copy_(Q[b]), fk.copy_(K[b])
            want = alignment.aligner_scores(Q[b].clone(), K[b].clone(), temperature=0.3)
            for first, (q, k) in enumerate(((Q[b], K[b]), (fq, fk))):
                ql, kl = q.detach().requires_grad_(True), k.detach().requires_grad_(True)
                s = alignment.aligner_scores(ql, kl, temperature=0.3)
                assert torch.equal(s.detach(), want), (C, off, b)
                (s * s).sum().backward()
                if first == 0:
                    ref = (ql.grad.clone(), kl.grad.clone())
                else:
                    assert torch.equal(ql.grad, ref[0]) and torch.equal(kl.grad, ref[1]), (C, off, b)


def _planted(seed):
    g = np.random.RandomState(seed)
    k = g.randn(40, 32).astype(np.float32)
    path = align_ref.random_path(g, 200, 40)
    q = (k[path] + np.float32(0.1) * g.randn(200, 32).astype(np.float32)).astype(np.float32)
    return q, k, path


def test_planted_path_is_recovered(native_lib):
    from tacotron2_amd import alignment
    q, k, path = _planted(0)
    assert np.array_equal(align_ref.align64(ar.scores64(q, k, 1.0)["s"].astype(np.float32))[2], path)      # the restatement recovers it
    s = alignment.aligner_scores(torch.from_numpy(q).to(DEV), torch.from_numpy(k).to(DEV), temperature=1.0)
    durations, _, got = alignment.monotonic_align(s, return_path=True)
    assert np.array_equal(got[0].cpu().numpy(), path) and np.array_equal(durations[0].cpu().numpy(), np.bincount(path, minlength=40))


def test_bench_tool_end_to_end(native_lib, tmp_path):
    out = tmp_path / "bench.json"
    r = subprocess.run([sys.executable, os.path.join(gu.ROOT, "tools", "bench_aligner.py"), "--cases", "tiny", "--reps", "1", "--inner", "2",
                        "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == json.loads(out.read_text()) and set(res["cases"]) == {"tiny"}
    c = res["cases"]["tiny"]
    assert c["error_over_allowed"]["s"] <= 1.0 and c["call_ms"]["forward"] > 0 and c["call_ms"]["forward_backward_loss"] > 0
    assert {"aligner_pack_keys_kernel", "aligner_rows_fwd_kernel", "aligner_z_kernel", "aligner_dq_kernel", "aligner_dk_kernel", "full_forward",
            "full_backward"} <= set(c["kernel_ms"]) and "torch_float32_forward_backward_ms" in c
