"""The length regulator on the MI355X (alignment.durations_to_path, alignment.length_regulate, alignment.LengthRegulator,
alignment.token_average, csrc/regulate.hip, the align tool's --token-features, tools/bench_regulate.py) against the restatements
of tests/regulate_ref.py: the cases and assertions of tests/test_regulate_cpu.py (tests/regulate_cases.py holds them) on the
device, and what only the device can show.

path, t_lengths, y, dx, num and den equal the float32 restatement bit for bit; the quotient m and dv are held to
``regulate_cases.MAX_ULPS`` of it; against float64, dx is within gamma_{m-1} sum |dy|, m within 2 [(gamma_m sum |w v| + |m64|
gamma_{m-1} sum w) / sum w + u |m64|] and dv within 2 |dv64| (gamma_{m-1} + 2 u), per element.  Every
case prints its figures (``FIGURE`` lines; profiles/regulate_pytest_gpu.txt has the run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
import regulate_cases as rc
import yin_cases as yc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("which", range(len(rc.SHAPES)))
def test_shapes(native_lib, which):
    rc.shape_case(which, DEV)


def test_limits_and_overflowing_sums(native_lib):
    from tacotron2_amd import native
    assert native.regulate_limits() == (512, 1024, 65536)
    rc.overflowing_sums(DEV)


def test_ragged_batch_equals_each_utterance_alone_and_two_calls_agree(native_lib):
    rc.ragged_equals_alone(DEV)


def test_more_utterances_than_compute_units(native_lib):
    rc.many_short(DEV)


def test_pooling_forms(native_lib):
    rc.pooling_forms(DEV)


def test_round_trip_with_monotonic_align(native_lib):
    rc.round_trip(DEV)


def test_planted_identity(native_lib):
    rc.planted_identity(DEV)


def test_autograd(native_lib):
    rc.autograd(DEV)


def test_refusals(native_lib):
    from tacotron2_amd import alignment, native
    rc.refusals(DEV)
    x, d = torch.zeros(1, 3, 2, device=DEV), torch.ones(1, 3, dtype=torch.int32, device=DEV)
    with pytest.raises(native.NativeError, match="no CPU path"):
        alignment.length_regulate(x.cpu(), d.cpu())
    with pytest.raises(ValueError, match="length_regulate: the tokens are on cuda:0 and the durations on cpu"):
        alignment.length_regulate(x, d.cpu(), None, 3)
    with pytest.raises(ValueError, match="token_average: the values are on cuda:0 and the durations on cpu"):
        alignment.token_average(torch.zeros(1, 3, device=DEV), d.cpu())
    with pytest.raises(ValueError, match="token_average: the values are on cuda:0 and the weights on cpu"):
        alignment.token_average(torch.zeros(1, 3, device=DEV), d, None, torch.ones(1, 3))


def test_the_longest_buffer(native_lib):
    """T = 65 536, the limit: one token owns 60 000 frames, the tail is cut."""
    from tacotron2_amd import alignment
    d = torch.tensor([[5, 60000, 0, 7000]], device=DEV)
    x = torch.tensor([[[1.0], [2.0], [3.0], [4.0]]], device=DEV).requires_grad_(True)
    y, tl = alignment.length_regulate(x, d, None, 65536)
    assert tl.tolist() == [65536] and torch.equal(y[0, :, 0], torch.repeat_interleave(x.detach()[0, :, 0], d[0])[:65536])
    y.sum().backward()
    assert x.grad[0, :, 0].tolist() == [5.0, 60000.0, 0.0, 5531.0]
    assert alignment.token_average(y.detach(), d)[0, :, 0].tolist() == [1.0, 2.0, 0.0, 4.0]


def _live():
    """The bytes asked of the allocator and not yet given back (its own blocks are up to 1 MiB larger than what was asked)."""
    return torch.cuda.memory_stats()["requested_bytes.all.current"]


def test_no_grad_keeps_the_outputs_alone_and_a_named_T_reads_nothing_back(native_lib):
    """Under no_grad what stays allocated after a call is the outputs; with T an int the call runs under torch's synchronisation
    debug mode set to 'error', which raises at any device-to-host copy and any other blocking call; with T = None the same mode
    reports the one read."""
    from tacotron2_amd import alignment
    B, N, C, T = 8, 100, 80, 400
    g = torch.Generator().manual_seed(0)
    d = torch.randint(0, 6, (B, N), generator=g).to(torch.int32).to(DEV)
    x, v, w = torch.randn(B, N, C, generator=g).to(DEV), torch.randn(B, T, C, generator=g).to(DEV), torch.rand(B, T, generator=g).to(DEV)
    n_dev = torch.full((B,), N, dtype=torch.int32, device=DEV)
    alignment.length_regulate(x, d, n_dev, T), alignment.token_average(v, d, n_dev, w)        # warm
    torch.cuda.synchronize()
    for leaf in (x, x.clone().requires_grad_(True)):
        before = _live()
        with torch.no_grad():
            y, tl = alignment.length_regulate(leaf, d, n_dev, T)
        torch.cuda.synchronize()
        assert _live() - before == 4 * B * T * C + 4 * B
        del y, tl
    before = _live()
    with torch.no_grad():
        m = alignment.token_average(v, d, n_dev, w)
    torch.cuda.synchronize()
    assert _live() - before == 4 * B * N * C
    before = _live()
    path, tl = alignment.durations_to_path(d, n_dev, T)
    torch.cuda.synchronize()
    assert _live() - before == 4 * B * T + 4 * B
    xl, vl = x.clone().requires_grad_(True), v.clone().requires_grad_(True)
    gy, gm = torch.randn(B, T, C, device=DEV), torch.randn(B, N, C, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        alignment.durations_to_path(d, n_dev, T)
        alignment.length_regulate(xl, d, n_dev, T)[0].backward(gy)
        alignment.token_average(vl, d, n_dev, w).backward(gm)
        alignment.LengthRegulator(max_len=T)(x, d, n_dev)
        with pytest.raises(RuntimeError, match="synchroniz"):
            alignment.length_regulate(x, d, n_dev)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert xl.grad is not None and vl.grad is not None


# ---- the tools -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fresh_checkpoint(tmp_path_factory):
    hpstr = gu.TINY_HP + ",max_decoder_steps=12"
    ckpt = tmp_path_factory.mktemp("regulate_ckpt") / "fresh.pt"
    torch.save({"iteration": 0, "state_dict": gu.build_state_dict(gu.make_hparams(hpstr), 1234), "optimizer": None,
                "learning_rate": 1e-3}, str(ckpt))
    return str(ckpt), hpstr


def test_align_tool_token_features_on_a_synthetic_filelist(native_lib, fresh_checkpoint, tmp_path, capsys):
    from tacotron2_amd import align
    ckpt, hpstr = fresh_checkpoint
    argv = ["--checkpoint", ckpt, "--filelist", "synthetic:8:5:40", "--hparams", hpstr, "--batch", "3"]
    plain = align.main(argv + ["-o", str(tmp_path / "plain")])
    old = capsys.readouterr().out
    more = align.main(argv + ["-o", str(tmp_path / "features"), "--token-features"])
    new = capsys.readouterr().out
    skipped = [ln for ln in new.splitlines() if ln.startswith("token features: pitch is skipped")]
    assert len(skipped) == 1 and "pitch" not in old
    # the decoder's prenet drops out in eval mode too, so two runs differ in their figures: the lines keep their names, counts and
    # fields, the summary its keys, the directory its listing
    fields = lambda text: [(ln.split()[:3], len(ln.split())) for ln in text.splitlines()[:-1] if not ln.startswith("token features")]   # noqa: E731
    assert fields(new) == fields(old)
    assert set(plain) == {"count", "focus_mean", "path_mass_mean", "off_path_mean", "backward_steps_mean", "max_duration_mean", "unalignable"}
    assert set(more) - set(plain) == {"energy_mean"} and set(plain) <= set(more) and more["energy_mean"] > 0
    assert (more["count"], more["unalignable"]) == (plain["count"], plain["unalignable"]) and plain["count"] >= 1
    names = sorted(os.listdir(str(tmp_path / "plain")))
    assert names == sorted(["summary.json"] + ["%d.npy" % i for i in range(8) if str(i) not in plain["unalignable"]])     # as before
    assert sorted(n for n in os.listdir(str(tmp_path / "features")) if not n.endswith(".energy.npy")) == names
    assert json.loads((tmp_path / "features" / "summary.json").read_text()) == more
    for n in names:
        if n != "summary.json":
            d, e = np.load(str(tmp_path / "features" / n)), np.load(str(tmp_path / "features" / (n[:-4] + ".energy.npy")))
            assert d.shape == np.load(str(tmp_path / "plain" / n)).shape and e.dtype == np.float32 and e.shape == d.shape and (e > 0).all()


def test_align_tool_token_features_on_wavs(native_lib, fresh_checkpoint, tmp_path, capsys):
    """Four wavs the test writes: two pulse trains (voiced), white noise, and a pulse train that stops half way."""
    from tacotron2_amd import align, audio
    from tacotron2_amd.utils import load_wav_to_torch
    ckpt, hpstr = fresh_checkpoint
    hp = gu.make_hparams(hpstr)
    n, sr = 256 * 30, 22050
    noise = np.random.RandomState(0).randn(n)
    half = np.concatenate([yc.pulse_train(150, n // 2), np.zeros(n - n // 2)])
    texts = {"pulse": "ids: 11 12", "noise": "ids: 11 12 13", "half": "ids: 5 6 7 8 9 10 11 12 13 14 15", "other": "ids: 11 1 12"}
    for name, sig in (("pulse", yc.pulse_train(100, n)), ("noise", noise), ("half", half), ("other", yc.pulse_train(220, n))):
        yc.write_wav(str(tmp_path / (name + ".wav")), sig, sr)
    filelist = tmp_path / "list.txt"
    filelist.write_text("".join("%s|%s\n" % (tmp_path / (k + ".wav"), t) for k, t in texts.items()))
    out = tmp_path / "out"
    summary = align.main(["--checkpoint", ckpt, "--filelist", str(filelist), "--hparams", hpstr, "--batch", "3", "-o", str(out), "--token-features"])
    printed = capsys.readouterr().out
    assert "pitch is skipped" not in printed and summary["count"] == 4 and summary["energy_mean"] > 0
    share, tokens = 0, 0
    for name in texts:
        d, e, f = (np.load(str(out / (name + suffix))) for suffix in (".npy", ".energy.npy", ".f0.npy"))
        assert f.dtype == np.float32 and f.shape == d.shape == e.shape and (f >= 0).all()
        share, tokens = share + int((f > 0).sum()), tokens + len(f)
        if name in ("pulse", "other"):
            want = sr / (100.0 if name == "pulse" else 220.0)                # pulse_train takes the period in samples
            assert f.any() and (np.abs(f[f > 0] - want) < 0.05 * want).all()
        wav = load_wav_to_torch(str(tmp_path / (name + ".wav")))[0] / hp.max_wav_value
        voiced = audio.yin(wav.to(DEV), None, sr=hp.sampling_rate, frame_length=hp.win_length, hop_length=hp.hop_length)[1][0].cpu().numpy()
        owner = np.repeat(np.arange(len(d)), d)
        has = np.array([voiced[:len(owner)][owner == k].any() for k in range(len(d))])
        assert np.array_equal(f > 0, has), name                             # zeros exactly on tokens without a voiced frame
    assert summary["f0_voiced_token_share"] == share / tokens and share > 0


def test_bench_tool_end_to_end(native_lib, tmp_path):
    out = tmp_path / "bench.json"
    r = subprocess.run([sys.executable, os.path.join(gu.ROOT, "tools", "bench_regulate.py"), "--cases", "tiny", "--reps", "1", "--inner", "2",
                        "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res == json.loads(out.read_text()) and set(res["cases"]) == {"tiny"}
    c = res["cases"]["tiny"]
    assert max(c["error_over_allowed"].values()) <= 1.0 and all(v > 0 for v in c["call_ms"].values())
    assert {"regulate_path_kernel", "regulate_expand_kernel", "regulate_segsum_kernel", "regulate_pool_kernel", "regulate_pool_bwd_kernel"} \
        == set(c["kernel_ms"]) and c["torch_gather_equals_y_bit_for_bit"] and "torch_float32_repeat_interleave_loop_ms" in c
