"""MCD-DTW on the MI355X (audio.mel_cepstrum, audio.dtw, audio.MelCepstralDistortion, csrc/dtw.hip) against the float64
restatement (tests/dtw_ref.py): the cases and assertions of tests/test_dtw_cpu.py (tests/dtw_cases.py holds them) on the device,
more workgroups than CUs, a pair that crosses several bands, and the evaluate tool's checkpoint mode.

The DTW cost is held to the derived bound (n_a + n_b + K + 8) 2^-24 relative to the float64 optimum over the same float32 cepstra
(DESIGN.md section 16); the cepstrum to 4 x the error float32 ``torch.matmul`` with the same basis shows against float64 in the same
test.  Every case prints its figures (``FIGURE`` lines; profiles/mcd_pytest_gpu.txt has the run)."""
import json
import os

import numpy as np
import pytest
import torch

import dtw_cases as dc
import dtw_ref as dr
import golden_util as gu

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("K", dc.KS)
@pytest.mark.parametrize("which", range(9))
def test_optimum_and_path(native_lib, which, K):
    n_a, n_b = dc.length_pairs()[which]
    dc.check_lengths(n_a, n_b, K, DEV)


def test_path_identity_where_the_optimum_is_unique_by_margin(native_lib):
    assert dc.margin_seeds(DEV) >= 8


def test_exact_ties_follow_the_tie_rule(native_lib):
    dc.tie_cases(DEV)


def test_ragged_batch_equals_each_pair_alone_and_two_calls_agree(native_lib):
    dc.ragged_equals_alone(dc.ragged_pairs(), DEV)


def test_module_equals_the_native_calls(native_lib):
    dc.module_equals_native(dc.ragged_pairs(K=5), DEV)


def test_more_workgroups_than_compute_units(native_lib):
    g = np.random.RandomState(21)
    pairs = [(g.randn(int(g.randint(1, 10)), 13).astype(np.float32), g.randn(int(g.randint(1, 10)), 13).astype(np.float32))
             for _ in range(300)]
    cost, steps, path = dc.run(pairs, DEV)
    again = dc.run(pairs, DEV, slab_check=False)
    assert np.array_equal(cost.view(np.int32), again[0].view(np.int32)) and np.array_equal(path, again[2])
    worst = 0.0
    for p, (a, b) in enumerate(pairs):
        opt, ref_steps, _ = dr.dtw(a, b)
        worst = max(worst, abs(float(cost[p]) - opt) / opt / dr.bound(a.shape[0], b.shape[0], 13))
        own = [tuple(int(v) for v in ij) for ij in path[p, :steps[p]]]
        assert abs(float(cost[p]) - opt) <= dr.bound(a.shape[0], b.shape[0], 13) * opt
        assert dr.is_warping_path(own, a.shape[0], b.shape[0]) and (path[p, steps[p]:] == -1).all()
        assert abs(dr.path_cost(a, b, own) - opt) <= dr.bound(a.shape[0], b.shape[0], 13) * opt
    print("\nFIGURE B=300 pairs of 1 to 9 frames: worst error / bound %.3f" % worst)


def test_a_pair_that_crosses_several_bands(native_lib):
    a, b = dr.sequences(513, 600, 13, 99)
    cost, steps, path = dc.run([(a, b)], DEV)
    dc.check_pair(a, b, cost[0], steps[0], path[0])
    again = dc.run([(a, b)], DEV, slab_check=False)
    assert cost.view(np.int32)[0] == again[0].view(np.int32)[0] and np.array_equal(path, again[2])


def test_mel_cepstrum_against_the_restatement(native_lib):
    errs = dc.cepstrum_errors(DEV)
    for K, (e_k, e_t) in errs.items():
        print("\nFIGURE cepstrum K=%d (80 mels, 257 frames, log-mel about -5 +- 2): kernel max abs error %.3e, float32 torch.matmul "
              "%.3e" % (K, e_k, e_t))
        assert e_k <= 4 * e_t


def test_mcd_end_to_end(native_lib):
    from tacotron2_amd import audio
    ma, mb = dc.stretched_mels()
    basis = torch.from_numpy(audio.cepstral_basis(80, 13)).to(DEV)
    e_t = max(np.abs(torch.matmul(torch.from_numpy(m).to(DEV).transpose(1, 2), basis.t()).cpu().double().numpy()
                     - dr.cepstrum(m)).max() for m in (ma, mb))
    print("\nFIGURE float32 torch.matmul cepstral error on the test's mels: %.3e" % e_t)
    dc.mcd_end_to_end(DEV, 4 * e_t * np.sqrt(13.0))
    mod = audio.MelCepstralDistortion(13, return_path=True).to(DEV)
    m = torch.from_numpy(ma).to(DEV)
    assert mod(m, m.clone()).item() == 0.0 and mod.last["steps"].item() == 120
    assert mod.last["path"].shape == (1, 239, 2) and mod.last["path"].grad_fn is None


def test_evaluate_checkpoint_mode(native_lib, tmp_path, capsys):
    from tacotron2_amd import evaluate
    hpstr = gu.TINY_HP + ",max_decoder_steps=12"
    ckpt = tmp_path / "fresh.pt"
    torch.save({"iteration": 0, "state_dict": gu.build_state_dict(gu.make_hparams(hpstr), 1234), "optimizer": None,
                "learning_rate": 1e-3}, str(ckpt))
    out = tmp_path / "mcd.json"
    summary = evaluate.main(["--checkpoint", str(ckpt), "--filelist", "synthetic:8:5:40", "--hparams", hpstr, "--batch", "3",
                             "-o", str(out)])
    lines = [ln for ln in capsys.readouterr().out.strip().splitlines() if ln.startswith("synthetic/") or ln.split()[0].isdigit()]
    assert json.loads(out.read_text()) == summary and summary["count"] == 8
    assert 0 <= summary["hit_max_decoder_steps"] <= 8
    rows = [ln.split() for ln in lines if len(ln.split()) == 5]
    assert len(rows) == 8 and sorted(r[0] for r in rows) == [str(i) for i in range(8)]
    for name, fa, fb, steps, db in rows:
        assert 1 <= int(fa) <= 12 and 2 <= int(fb) <= 40 and max(int(fa), int(fb)) <= int(steps) <= int(fa) + int(fb) - 1
        assert np.isfinite(float(db)) and float(db) > 0.0
    for key in ("mcd_db_mean", "mcd_db_std", "mcd_db_median", "length_ratio_mean"):
        assert np.isfinite(summary[key])
