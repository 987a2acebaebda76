"""YIN on the MI355X (audio.yin, audio.f0_metrics, csrc/yin.hip, the evaluate tool's wav mode) against the float64 restatement
(tests/yin_ref.py): the cases and assertions of tests/test_yin_cpu.py (tests/yin_cases.py holds them) on the device, more
workgroups than CUs, and the tool end to end.

d' of every lag of every frame is held to the derived bound (2 W + tau_max + 8) 2^-24 relative to the restatement (DESIGN.md
section 17.3); the choice of lag is exact given the kernel's own d', and equal to the restatement's wherever the restatement's
decision keeps its margin under that bound.  Every case prints its figures (``FIGURE`` lines; profiles/yin_pytest_gpu.txt has the
run)."""
import json
import os

import numpy as np
import pytest
import torch

import dtw_cases as dc
import golden_util as gu
import yin_cases as yc
import yin_ref as yr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def test_exact_periods(native_lib):
    yc.periodic_structure(DEV)


def test_default_geometry_glides(native_lib):
    yc.check_batch(yc.glide_signals(), DEV, yc.DEFAULT, "glides", min_decided=0.90)


@pytest.mark.parametrize("offset", range(4))
def test_small_geometry_at_every_alignment(native_lib, offset):
    yc.check_batch(yc.small_signals(), DEV, yc.SMALL, "small+%d" % offset, offset=offset)


@pytest.mark.parametrize("name", ["ODD", "TAIL", "LONG"])
def test_other_geometries(native_lib, name):
    geo = getattr(yc, name)
    g = np.random.RandomState(5)
    n = 5 * geo["hop_length"] + 3
    signals = [yr.periodic(geo["frame_length"] // 4 - 3, n, 4), g.randn(n - geo["hop_length"]).astype(np.float32)]
    yc.check_batch(signals, DEV, geo, name, offset=1)


def test_all_zero(native_lib):
    yc.all_zero(DEV)
    yc.all_zero(DEV, yc.ODD)


def test_ragged_batch_equals_each_utterance_alone_and_two_calls_agree(native_lib):
    yc.ragged_equals_alone(yc.small_signals(), DEV, yc.SMALL)
    yc.ragged_equals_alone(yc.glide_signals()[:2] + [yr.periodic(100, 3000)], DEV, yc.DEFAULT, offset=2)


def test_module_equals_the_native_calls(native_lib):
    yc.module_equals_native(yc.small_signals()[:5], DEV, yc.SMALL)
    yc.module_equals_native(yc.glide_signals()[:2], DEV, yc.DEFAULT)


def test_more_workgroups_than_compute_units(native_lib):
    g = np.random.RandomState(21)
    signals = [g.randn(int(g.randint(1, 100))).astype(np.float32) for _ in range(300)]
    yc.check_batch(signals, DEV, yc.SMALL, "300 short utterances", offset=3)


def test_f0_metrics(native_lib):
    yc.check_metrics(DEV)


def test_refusals(native_lib):
    yc.refusals(DEV)


# ---- the tool ----------------------------------------------------------------------------------------------------------------
def _rows(lines):
    return dict((ln.split()[0], ln.split()[1:]) for ln in lines if ".wav " in ln and not ln.startswith("unmatched"))


def test_evaluate_wavs(native_lib, tmp_path, capsys):
    from tacotron2_amd import evaluate
    da, db, dc_ = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (da, db, dc_):
        d.mkdir()
    n = 5120
    for d in (da, db):
        yc.write_wav(str(d / "pulse.wav"), yc.pulse_train(100, n), 22050)
        yc.write_wav(str(d / "glide.wav"), yr.glide(0), 22050)
    yc.write_wav(str(da / "only_a.wav"), yc.pulse_train(100, n), 22050)
    (db / "notes.txt").write_text("not a wav")
    out = tmp_path / "f0.json"
    summary = evaluate.main(["--wavs", str(da), str(db), "-o", str(out)])
    lines = capsys.readouterr().out.strip().splitlines()
    assert json.loads(lines[-1]) == summary == json.loads(out.read_text())
    assert summary["count"] == 2 and summary["unmatched"] == ["only_a.wav"] and "unmatched (only in A): only_a.wav" in lines
    assert summary["mcd_db_mean"] == 0.0 and summary["f0_rmse_cents_mean"] == 0.0 and summary["f0_rmse_cents_median"] == 0.0
    assert summary["vuv_error_mean"] == 0.0 and summary["gross_pitch_error_mean"] == 0.0 and summary["no_voiced_overlap"] == 0
    assert abs(summary["f0_corr_mean"] - 1.0) <= 1e-9
    rows = _rows(lines)
    assert rows["pulse.wav"][:4] == ["21", "21", "21", "0.0000"] and rows["pulse.wav"][4] == "0.000" and len(rows["pulse.wav"]) == 9
    assert int(rows["pulse.wav"][8]) >= 17 and int(rows["glide.wav"][8]) >= 5

    # the same pulse at another exact period: the sign and size of the pitch shift, within half a lag on either side
    yc.write_wav(str(dc_ / "pulse.wav"), yc.pulse_train(110, n), 22050)
    summary = evaluate.main(["--wavs", str(da), str(dc_)])
    lines = capsys.readouterr().out.strip().splitlines()
    cents = float(_rows(lines)["pulse.wav"][4])
    with capsys.disabled():
        print("\nFIGURE period 100 against period 110: %.3f cents, exact ratio %.3f" % (cents, 1200 * np.log2(1.1)))
    assert 1200 * np.log2(109.5 / 100.5) <= cents <= 1200 * np.log2(110.5 / 99.5)
    assert summary["count"] == 1 and summary["f0_rmse_cents_mean"] == pytest.approx(cents, abs=1e-3)
    assert summary["gross_pitch_error_mean"] == 0.0 and summary["mcd_db_mean"] > 0
    # a root mean square carries no sign: swapped, the same size (the path may pair other frames)
    swapped = evaluate.main(["--wavs", str(dc_), str(da)])
    capsys.readouterr()
    assert swapped["f0_rmse_cents_mean"] == pytest.approx(cents, abs=0.5)

    yc.write_wav(str(dc_ / "pulse.wav"), yc.pulse_train(110, n), 16000)
    with pytest.raises(ValueError, match="sampling rate 16000, expected 22050"):
        evaluate.main(["--wavs", str(da), str(dc_)])


def test_evaluate_mels_prints_what_it_printed_before(native_lib, tmp_path, capsys):
    """The --mels summary of a fixed pair, byte for byte what the parent commit printed (tests/golden/evaluate_mels_summary.txt
    was recorded with the parent's evaluate.py on the MI355X)."""
    from tacotron2_amd import evaluate
    ma, mb = dc.stretched_mels(n_mel=80, T=60)
    da, db = tmp_path / "a", tmp_path / "b"
    da.mkdir()
    db.mkdir()
    np.save(str(da / "x.npy"), ma[0])
    np.save(str(db / "x.npy"), mb[0])
    np.save(str(da / "same.npy"), ma[0])
    np.save(str(db / "same.npy"), ma[0])
    evaluate.main(["--mels", str(da), str(db)])
    got = capsys.readouterr().out
    with open(os.path.join(gu.ROOT, "tests", "golden", "evaluate_mels_summary.txt")) as fh:
        assert got == fh.read()
