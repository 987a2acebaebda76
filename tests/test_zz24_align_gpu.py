"""Forced alignment on the MI355X (alignment.monotonic_align, alignment.attention_durations, csrc/align.hip, the align tool and
the evaluate tool's --alignment flag) against the restatements (tests/align_ref.py): the cases and assertions of
tests/test_align_cpu.py (tests/align_cases.py holds them) on the device, more workgroups than CUs, and the tools end to end.

Score, durations and path equal the float32 restatement bit for bit (the recurrence is one IEEE add per cell).  The returned
path's float64 score lies within (T + 2) 2^-24 S of the float64 optimum, S the summed magnitude of the path's scores, and the
float32 score within the same of the returned path's.  Every case prints its figures (``FIGURE`` lines;
profiles/align_pytest_gpu.txt has the run)."""
import json

import numpy as np
import pytest
import torch

import align_cases as ac
import align_ref as ar
import golden_util as gu

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("kind", ac.KINDS)
@pytest.mark.parametrize("which", range(len(ac.SHAPES)))
def test_shapes(native_lib, which, kind):
    ac.check_shape(*ac.SHAPES[which], kind, DEV)


def test_exact_ties_follow_the_tie_rule(native_lib):
    ac.ties(DEV)


def test_planted_path_comes_back(native_lib):
    ac.planted(DEV)


def test_ragged_batch_equals_each_utterance_alone_and_two_calls_agree(native_lib):
    ac.ragged_equals_alone(ac.ragged_mats(), DEV)


def test_module_equals_the_native_calls(native_lib):
    ac.module_equals_native(ac.ragged_mats(), DEV)


def test_more_workgroups_than_compute_units(native_lib):
    ac.many_short(DEV)


def test_attention_durations(native_lib):
    ac.attention_case(DEV)


def test_walk_stays_inside_whatever_the_scores(native_lib):
    g = np.random.RandomState(9)
    x = ar.mixed_sign(g, 40, 17)
    x[g.rand(40, 17) < 0.2] = np.nan
    x[g.rand(40, 17) < 0.2] = np.inf
    ac.run([x, np.full((30, 30), -np.inf, np.float32)], DEV)


def test_refusals(native_lib):
    from tacotron2_amd import alignment, native
    ac.refusals(DEV)
    with pytest.raises(native.NativeError, match="no CPU path"):
        alignment.monotonic_align(torch.zeros(1, 4, 2))


# ---- the tools -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fresh_checkpoint(tmp_path_factory):
    hpstr = gu.TINY_HP + ",max_decoder_steps=12"
    ckpt = tmp_path_factory.mktemp("align_ckpt") / "fresh.pt"
    torch.save({"iteration": 0, "state_dict": gu.build_state_dict(gu.make_hparams(hpstr), 1234), "optimizer": None,
                "learning_rate": 1e-3}, str(ckpt))
    return str(ckpt), hpstr


def test_align_tool(native_lib, fresh_checkpoint, tmp_path, capsys):
    from tacotron2_amd import align
    from tacotron2_amd.data_utils import TextMelLoader
    ckpt, hpstr = fresh_checkpoint
    out = tmp_path / "durations"
    summary = align.main(["--checkpoint", ckpt, "--filelist", "synthetic:8:5:40", "--hparams", hpstr, "--batch", "3", "-o", str(out)])
    lines = capsys.readouterr().out.strip().splitlines()
    assert json.loads(lines[-1]) == summary == json.loads((out / "summary.json").read_text())
    assert set(summary) == {"count", "focus_mean", "path_mass_mean", "off_path_mean", "backward_steps_mean", "max_duration_mean",
                            "unalignable"}
    data = TextMelLoader("synthetic:8:5:40", gu.make_hparams(hpstr))
    rows = dict((ln.split()[0], ln.split()[1:]) for ln in lines[:-1] if not ln.startswith("unalignable"))
    assert summary["count"] == len(rows) and summary["count"] + len(summary["unalignable"]) == 8 and summary["count"] >= 1
    for i in range(8):
        text, mel = data[i]
        name = data.audiopaths_and_text[i][0].split('/')[1]                 # the loader shuffles its list
        if text.numel() > mel.shape[1]:
            assert name in summary["unalignable"]
            continue
        d = np.load(str(out / (name + ".npy")))
        assert d.dtype == np.int32 and d.shape == (text.numel(),) and d.sum() == mel.shape[1] and d.min() >= 1
        tokens, frames, focus, mass, off, back, longest = rows[name]
        assert (int(tokens), int(frames)) == (text.numel(), mel.shape[1]) and int(longest) == d.max()
        assert 0.0 < float(mass) <= float(focus) <= 1.0 and 0.0 <= float(off) <= 1.0 and 0 <= int(back) < int(frames)
    for key in ("focus_mean", "path_mass_mean", "off_path_mean", "backward_steps_mean", "max_duration_mean"):
        assert np.isfinite(summary[key])


def test_evaluate_checkpoint_with_and_without_alignment(native_lib, fresh_checkpoint, capsys):
    from tacotron2_amd import evaluate
    ckpt, hpstr = fresh_checkpoint
    argv = ["--checkpoint", ckpt, "--filelist", "synthetic:8:5:40", "--hparams", hpstr, "--batch", "3"]
    plain = evaluate.main(argv)
    old = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()[:-1] if not ln.startswith("Warning")]
    assert len(old) == 8 and all(len(r) == 5 for r in old)                  # the five fields of before, nothing else
    assert set(plain) == {"count", "mcd_db_mean", "mcd_db_std", "mcd_db_median", "length_ratio_mean", "hit_max_decoder_steps"}
    more = evaluate.main(argv + ["--alignment"])
    new = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()[:-1] if not ln.startswith("Warning")]
    assert sorted(r[0] for r in new) == sorted(r[0] for r in old) == [str(i) for i in range(8)] and set(plain) <= set(more)
    assert set(more) - set(plain) == {"focus_mean", "path_mass_mean", "off_path_mean", "backward_steps_mean", "max_duration_mean",
                                     "unalignable"}
    assert all(len(r) == 10 or r[5:] == ["unalignable"] for r in new)
    assert more["unalignable"] == sum(1 for r in new if r[5:] == ["unalignable"])
    for r in new:
        if len(r) == 10:                                                    # a decode at least as long as its text
            assert 0.0 < float(r[6]) <= float(r[5]) <= 1.0 and 0.0 <= float(r[7]) <= 1.0 and 1 <= int(r[9]) <= int(r[1])
