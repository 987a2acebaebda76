"""The forward-sum alignment likelihood on the MI355X (alignment.forward_sum, alignment.alignment_posterior,
alignment.ForwardSumLoss, csrc/forward_sum.hip, the --posterior flag of the align and evaluate tools) against the float64
restatement (tests/forward_sum_ref.py): the cases and assertions of tests/test_forward_sum_cpu.py (tests/forward_sum_cases.py holds
them) on the device, more workgroups than CUs, autograd, and the tools end to end.

Per case the allowed error of log Z, gamma (largest absolute) and the soft durations is 4 x the float32 restatement's own error on
that case, computed here on the CPU, and at least 8 2^-24 max(1, |log Z|) for log Z and 8 2^-24 for gamma and the durations
(DESIGN.md section 19.4).  Every case prints its ratios error / allowed (``FIGURE`` lines; profiles/forward_sum_pytest_gpu.txt has
the run)."""
import json

import numpy as np
import pytest
import torch

import forward_sum_cases as fc
import forward_sum_ref as fr
import golden_util as gu
from test_forward_sum_cpu import ctc_neg_log_z

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _viterbi(x):
    from tacotron2_amd import alignment
    return alignment.monotonic_align(torch.from_numpy(np.array(x)).to(DEV))[1][0].item()


@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("which", range(len(fc.SHAPES)))
def test_shapes(native_lib, which, kind):
    fc.check_shape(*fc.SHAPES[which], kind, DEV, viterbi=_viterbi)          # and section 18's score <= log Z


def test_ragged_batch_equals_each_utterance_alone_and_two_calls_agree(native_lib):
    fc.ragged_equals_alone(fc.ragged_mats(), DEV)


def test_module_equals_the_native_calls_and_autograd(native_lib):
    fc.module_equals_native(fc.ragged_mats(), DEV)
    fc.loss_module(fc.ragged_mats(), DEV)


def test_more_workgroups_than_compute_units(native_lib):
    fc.many_short(DEV)


def test_planted_path_holds_the_posterior(native_lib):
    fc.planted(DEV)


def test_all_zero_scores_count_the_paths(native_lib):
    fc.all_zero(DEV)


def test_impossible_cells(native_lib):
    fc.impossible(DEV)


def test_non_finite_scores_leave_the_poison_intact(native_lib):
    fc.non_finite(DEV)


def test_refusals(native_lib):
    from tacotron2_amd import alignment, native
    fc.refusals(DEV)
    with pytest.raises(native.NativeError, match="no CPU path"):
        alignment.forward_sum(torch.zeros(1, 4, 2))


def test_loss_behind_a_log_softmax_against_float64_ctc_loss(native_lib):
    """ForwardSumLoss('sum') of log_softmax(logits) on the device against float64 F.ctc_loss (blank of -inf) of the float64
    log_softmax of the same logits on the CPU.  The loss is held to the case's log Z tolerance plus T 8 2^-24 max|l| for the
    float32 log_softmax feeding the kernel (each score within a few 2^-24 |l|, log Z moves by at most their sum along a path).
    The gradient with respect to the logits is -(gamma(t,n) - p(t,n) sum_k gamma(t,k)): with every gamma within tg that is within
    tg + p N tg <= tg (1 + N), plus N 8 2^-24 for the float32 softmax forward and backward on the device."""
    from tacotron2_amd import alignment
    for T, N in ((65, 64), (130, 63), (296, 257)):
        g = torch.Generator().manual_seed(T)
        logits = (3.0 * torch.randn(T, N, generator=g))
        leaf = logits.to(DEV).requires_grad_(True)
        loss = alignment.ForwardSumLoss('sum')(torch.log_softmax(leaf, dim=1))
        loss.backward()
        ref_leaf = logits.double().requires_grad_(True)
        lp = torch.log_softmax(ref_leaf, dim=1)
        want = torch.nn.functional.ctc_loss(torch.cat([torch.full((T, 1), -np.inf, dtype=torch.float64), lp], dim=1).unsqueeze(1),
                                            torch.arange(1, N + 1).unsqueeze(0), torch.tensor([T]), torch.tensor([N]), blank=0,
                                            reduction='sum')
        want.backward()
        x = lp.detach().float().numpy()
        tz, tg, _ = fc.allowed(fr.forward_sum32(x), fr.forward_sum64(x))
        assert abs(float(ctc_neg_log_z(x)[0]) - fr.forward_sum64(x)[0] * -1.0) <= 1e-9 * T
        e_loss = abs(float(loss.detach()) - float(want.detach()))
        e_grad = float((leaf.grad.cpu().double() - ref_leaf.grad).abs().max())
        b_loss, b_grad = tz + T * 8 * fr.U * float(np.abs(x).max()), tg * (1 + N) + N * 8 * fr.U
        print("FIGURE loss behind log_softmax (%d, %d): loss error %.3g (allowed %.3g), gradient error %.3g (allowed %.3g)"
              % (T, N, e_loss, b_loss, e_grad, b_grad))
        assert e_loss <= b_loss and e_grad <= b_grad, (T, N)


def test_no_grad_allocates_no_slab(native_lib):
    from tacotron2_amd import alignment, native
    B, T, N = 4, 700, 300
    x = torch.randn(B, T, N, device=DEV)
    alignment.forward_sum(x)                                                # the allocator's pools are warm
    torch.cuda.synchronize()
    slab = native.forward_sum_workspace(B, T, N, True)
    assert slab > 4 * B * T * N and native.forward_sum_workspace(B, T, N, False) == 16 * B
    for leaf, kept in ((x, False), (x.clone().requires_grad_(True), True)):
        for grad_mode in (False, True):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            with torch.set_grad_enabled(grad_mode):
                out = alignment.forward_sum(leaf)
            torch.cuda.synchronize()
            peak, after = torch.cuda.max_memory_allocated() - before, torch.cuda.memory_allocated() - before
            if kept and grad_mode:
                assert out.grad_fn is not None and after >= slab
            else:
                assert out.grad_fn is None and peak < slab // 8 and after < slab // 8, (kept, grad_mode, peak, after)
            del out


# ---- the tools -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fresh_checkpoint(tmp_path_factory):
    hpstr = gu.TINY_HP + ",max_decoder_steps=12"
    ckpt = tmp_path_factory.mktemp("forward_sum_ckpt") / "fresh.pt"
    torch.save({"iteration": 0, "state_dict": gu.build_state_dict(gu.make_hparams(hpstr), 1234), "optimizer": None,
                "learning_rate": 1e-3}, str(ckpt))
    return str(ckpt), hpstr


PLAIN_KEYS = {"count", "focus_mean", "path_mass_mean", "off_path_mean", "backward_steps_mean", "max_duration_mean", "unalignable"}
NEW_KEYS = {"log_likelihood_per_frame_mean", "path_log_posterior_per_frame_mean"}


def test_align_tool_posterior(native_lib, fresh_checkpoint, tmp_path, capsys):
    from tacotron2_amd import align
    ckpt, hpstr = fresh_checkpoint
    argv = ["--checkpoint", ckpt, "--filelist", "synthetic:8:5:40", "--hparams", hpstr, "--batch", "3"]
    plain = align.main(argv + ["-o", str(tmp_path / "plain")])
    old = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()[:-1] if not ln.startswith("unalignable")]
    assert set(plain) == PLAIN_KEYS and all(len(r) == 8 for r in old) and not list((tmp_path / "plain").glob("*.soft.npy"))
    out = tmp_path / "posterior"
    summary = align.main(argv + ["-o", str(out), "--posterior"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert json.loads(lines[-1]) == summary == json.loads((out / "summary.json").read_text())
    assert set(summary) - PLAIN_KEYS == NEW_KEYS and PLAIN_KEYS <= set(summary)     # (the prenet's dropout differs between runs)
    rows = [ln.split() for ln in lines[:-1] if not ln.startswith("unalignable")]
    assert len(rows) == summary["count"] >= 1 and [r[:3] for r in rows] == [r[:3] for r in old] and all(len(r) == 10 for r in rows)
    for r in rows:
        frames = int(r[2])
        hard, soft = np.load(str(out / (r[0] + ".npy"))), np.load(str(out / (r[0] + ".soft.npy")))
        assert soft.dtype == np.float32 and soft.shape == hard.shape and abs(float(soft.sum()) - frames) <= 1e-3 * frames
        assert float(r[9]) <= 1e-4 and np.isfinite(float(r[8]))            # the path's log posterior per frame is <= 0
    assert summary["path_log_posterior_per_frame_mean"] <= 1e-4 and np.isfinite(summary["log_likelihood_per_frame_mean"])
    assert len(list(out.glob("*.soft.npy"))) == len(rows)


def test_evaluate_alignment_posterior(native_lib, fresh_checkpoint, capsys):
    from tacotron2_amd import evaluate
    ckpt, hpstr = fresh_checkpoint
    argv = ["--checkpoint", ckpt, "--filelist", "synthetic:8:5:40", "--hparams", hpstr, "--batch", "3", "--alignment"]
    plain = evaluate.main(argv)
    old = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()[:-1] if not ln.startswith("Warning")]
    more = evaluate.main(argv + ["--posterior"])
    new = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()[:-1] if not ln.startswith("Warning")]
    assert set(more) - set(plain) == NEW_KEYS and set(plain) <= set(more)
    assert all(len(r) == 10 or r[5:] == ["unalignable"] for r in old)
    assert all(len(r) == 12 or r[5:] == ["unalignable"] for r in new) and sorted(r[0] for r in new) == sorted(r[0] for r in old)
    for r in new:
        if len(r) == 12:
            assert float(r[11]) <= 1e-4 and np.isfinite(float(r[10]))
