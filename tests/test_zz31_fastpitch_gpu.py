"""The thin ends of a temporal predictor, the predictor, FastPitch and its loss on the MI355X (fastpitch.channel_project,
fastpitch.scalar_embed, TemporalPredictor, FastPitch, FastPitchLoss, csrc/predictor_rows.hip) against the float64 restatements
(tests/predictor_ref.py, tests/predictor_cases.py).

Per case and per tensor the largest absolute error over the utterance's region is at most
max(4 x the float32 restatement's own largest error on that case, 8 2^-24 max(1, largest |value| of that tensor in float64))
(DESIGN.md sections 19.4 / 20.4 / 22.4 / 23.4 / 24.4).  Every case prints its ratios error / allowed (``FIGURE`` lines;
profiles/fastpitch_pytest_gpu.txt has the run)."""
import math

import numpy as np
import pytest
import torch

import predictor_cases as pc
import predictor_ref as pr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32 = np.float32


# ---- the two thin ops ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", pc.PROJECT_T)
@pytest.mark.parametrize("P", pc.PROJECT_P)
@pytest.mark.parametrize("C", pc.PROJECT_C)
def test_projection_shapes(native_lib, C, P, T):
    """y, dh, dw and db, with and without a bias, at T > T_b and a shifted base."""
    for bias in (False, True):
        batch = pc.project_batch((T,), C, P, bias)
        pc.check_project(batch, pc.run_project(batch, DEV, T=T + 1 + T % 3, offset=1 + T % 2))


@pytest.mark.parametrize("T", pc.EMBED_T)
@pytest.mark.parametrize("shape", pc.EMBED_SHAPES)
def test_embedding_shapes(native_lib, shape, T):
    """y, dbase, dv, dw and db, with and without a bias and a base; at k = 9 the utterances of 1 to 4 frames put every tap outside
    the utterance at some frame."""
    for bias in (False, True):
        for base in (False, True):
            batch = pc.embed_batch((T,), *shape, bias, base)
            pc.check_embed(batch, pc.run_embed(batch, DEV, T=T + 1 + T % 3, offset=1 + T % 2))


def test_ragged_batch_equals_each_utterance_alone_and_two_calls_agree(native_lib):
    """Six utterances of (0, 1, 2, 5, 128, 130) frames with NaN beyond T_b in every operand and the gradient: exact +0 in the
    padding (inside the checks), the bits of each utterance alone at another T and base offset, and the same bits from a second
    call."""
    proj = pc.project_batch(pc.RAGGED, 384, 2, True)
    emb = pc.embed_batch(pc.RAGGED, 384, 2, 3, True, True)
    for batch, run, check, per_row in ((proj, pc.run_project, pc.check_project, ("y", "dh")),
                                       (emb, pc.run_embed, pc.check_embed, ("y", "dv", "dbase"))):
        first, again = run(batch, DEV, T=131), run(batch, DEV, T=131)
        check(batch, first, "ragged ")
        for n in first:
            if n != "T":
                assert np.array_equal(pc.bits(first[n]), pc.bits(again[n])), n
        for b, u in enumerate(batch["utts"]):
            if u["T"]:
                alone = run(dict(batch, utts=[u]), DEV, T=u["T"] + b % 2, offset=1 + b % 3)
                for n in per_row:
                    assert np.array_equal(pc.bits(first[n][b, :u["T"]]), pc.bits(alone[n][0, :u["T"]])), (b, n)


def test_sums_across_many_short_utterances(native_lib):
    """300 utterances of 1 to 11 frames: 3300 rows in 52 partial sums."""
    Ts = tuple(1 + i % 11 for i in range(300))
    assert pr.sum_plan(300, 11) == (52, 64)
    batch = pc.project_batch(Ts, 32, 4, True)
    pc.check_project(batch, pc.run_project(batch, DEV), "300 utterances ")
    batch = pc.embed_batch(Ts, 32, 2, 3, True, True)
    pc.check_embed(batch, pc.run_embed(batch, DEV), "300 utterances ")


# ---- the modules ---------------------------------------------------------------------------------------------------------------
def _figure(label, got, f32, f64):
    worst = {}
    for n in got:
        pairs = zip(got[n], f32[n], f64[n]) if isinstance(got[n], list) else [(got[n], f32[n], f64[n])]
        for a, r32, r64 in pairs:
            worst[n] = max(worst.get(n, 0.0), pr.error(a, r64) / pr.allowed(r32, r64))
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:6]
    print("FIGURE predictor module %s: error / allowed, worst of %d tensors: %s" % (label, len(worst), " ".join("%s %.3f" % kv for kv in top)))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}


def test_temporal_predictor(native_lib):
    """Two predictions per token on (3, 7, 12) tokens against the torch run on each utterance alone; output and every parameter
    gradient; +0 beyond every length."""
    from tacotron2_amd import fastpitch
    torch.manual_seed(3)
    module = fastpitch.TemporalPredictor(64, 64, 3, n_layers=2, n_predictions=2)
    with torch.no_grad():
        for p in module.parameters():
            p.add_(0.05 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in module.state_dict().items()}
    module = module.to(DEV)
    r = np.random.default_rng(9)
    xs = [r.standard_normal((t, 64)).astype(F32) for t in pc.TOKENS]
    gs = [r.standard_normal((t, 2)).astype(F32) for t in pc.TOKENS]
    lengths = torch.tensor(pc.TOKENS, dtype=torch.int32, device=DEV)
    out = module(pc.layout(xs, DEV, 13), lengths)
    assert tuple(out.shape) == (3, 13, 2)
    for b, t in enumerate(pc.TOKENS):
        assert not out.detach()[b, t:].view(torch.int32).any()
    out.backward(pc.layout(gs, DEV, 13))
    got = dict(out=[out.detach()[b, :t].cpu().numpy() for b, t in enumerate(pc.TOKENS)])
    got.update({n: p.grad.cpu().numpy() for n, p in module.named_parameters()})
    refs = {}
    for dtype in (torch.float64, torch.float32):
        leaves = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
        outs = [pc.predictor_ref(leaves, "", torch.from_numpy(a).to(dtype)) for a in xs]
        sum((o * torch.from_numpy(g).to(dtype)).sum() for o, g in zip(outs, gs)).backward()
        refs[dtype] = dict(out=[o.detach().numpy() for o in outs])
        refs[dtype].update({n: leaves[n].grad.numpy() for n in leaves})
    _figure("TemporalPredictor", got, refs[torch.float32], refs[torch.float64])
    one = fastpitch.TemporalPredictor(64, 64, 3).to(DEV)
    assert tuple(one(pc.layout(xs, DEV, 13), lengths).shape) == (3, 13)


def _reference(sd, utts, dtype):
    """FastPitch.forward and FastPitchLoss in torch on each utterance alone -> outputs, the loss and every parameter gradient."""
    leaves = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    mels, durs, pitches = [], [], []
    se = dict(mel=0.0, duration=0.0, pitch=0.0)
    for u in utts:
        enc, log_dur, pitch_pred = pc.encode_ref(leaves, pc.SMALL, torch.from_numpy(u["ids"]))
        mel = pc.decode_ref(leaves, pc.SMALL, enc, u["durations"], torch.from_numpy(u["pitch"]))
        se["mel"] = se["mel"] + ((mel - torch.from_numpy(u["mel"]).to(dtype)) ** 2).sum()
        se["duration"] = se["duration"] + ((log_dur - torch.log1p(torch.from_numpy(u["durations"]).to(dtype))) ** 2).sum()
        se["pitch"] = se["pitch"] + ((pitch_pred - torch.from_numpy(u["pitch"]).to(dtype)) ** 2).sum()
        mels.append(mel), durs.append(log_dur), pitches.append(pitch_pred)
    frames, tokens = sum(u["T"] for u in utts), sum(u["N"] for u in utts)
    total = se["mel"] / (frames * pc.SMALL["n_mel"]) + 0.1 * se["duration"] / tokens + 0.1 * se["pitch"] / tokens
    total.backward()
    out = dict(mel=[m.detach().numpy() for m in mels], log_dur=[d.detach().numpy() for d in durs],
               pitch_pred=[p.detach().numpy() for p in pitches], loss=total.detach().numpy())
    out.update({"grad " + n: (leaves[n].grad if leaves[n].grad is not None else torch.zeros_like(leaves[n])).numpy() for n in leaves})
    return out


def _device_batch(utts, nan_pitch=True):
    text = pc.pad_tokens(utts, "ids", DEV, torch.long)
    dur = pc.pad_tokens(utts, "durations", DEV, torch.int32, fill=3)        # what lies beyond N_b is ignored
    pitch = pc.pad_tokens(utts, "pitch", DEV, torch.float32, fill=float("nan") if nan_pitch else 0.0)
    return text, dur, pitch


def test_fastpitch_forward_backward_with_its_loss(native_lib):
    """The small model (d_model 64, 2 layers, 1 head of 32, d_inner 128, filter 64, n_mel 80, 11 symbols) on tokens (3, 7, 12) with
    durations 0 to 4 and a zero-duration token: every output, the loss and every parameter gradient of FastPitchLoss; the float32
    restatement is the float32 torch run per utterance alone, the float64 the same in double."""
    from tacotron2_amd import fastpitch
    model, sd = pc.small_model()
    model = model.to(DEV)
    utts = pc.small_batch()
    text, dur, pitch = _device_batch(utts)
    T = max(u["T"] for u in utts)
    out = model(text, dur, pitch)
    mel, t_lengths, log_dur, pitch_pred, energy_pred = out
    assert energy_pred is None and tuple(mel.shape) == (3, T, 80) and t_lengths.tolist() == [u["T"] for u in utts]
    for b, u in enumerate(utts):
        assert not mel.detach()[b, u["T"]:].view(torch.int32).any()
        assert not log_dur.detach()[b, u["N"]:].view(torch.int32).any() and not pitch_pred.detach()[b, u["N"]:].view(torch.int32).any()
    target = pc.layout([u["mel"] for u in utts], DEV, T + 2)
    total, parts = fastpitch.FastPitchLoss()(out, target, dur, pitch, None, torch.tensor(pc.TOKENS, device=DEV))
    total.backward()
    got = dict(mel=[mel.detach()[b, :u["T"]].cpu().numpy() for b, u in enumerate(utts)],
               log_dur=[log_dur.detach()[b, :u["N"]].cpu().numpy() for b, u in enumerate(utts)],
               pitch_pred=[pitch_pred.detach()[b, :u["N"]].cpu().numpy() for b, u in enumerate(utts)], loss=total.detach().cpu().numpy())
    got.update({"grad " + n: p.grad.cpu().numpy() for n, p in model.named_parameters()})
    f64, f32 = _reference(sd, utts, torch.float64), _reference(sd, utts, torch.float32)
    assert set(got) == set(f64)
    _figure("FastPitch forward + backward", got, f32, f64)
    mel_part, dur_part, pitch_part = (float(parts[n].detach()) for n in ("mel", "duration", "pitch"))
    assert abs(mel_part + 0.1 * dur_part + 0.1 * pitch_part - float(total.detach())) <= 1e-5 * float(total.detach())


INFER_SEED = 11


def _infer_model():
    model, sd = pc.small_model(INFER_SEED, dur_bias=math.log(4.0))
    return model.to(DEV), sd


def test_infer_durations_equal_the_float64_reference_and_its_mel_equals_forward(native_lib):
    model, sd = _infer_model()
    utts = pc.small_batch()
    text, _, _ = _device_batch(utts)
    for pace in (1.0, 2.0):
        want = pc.infer_reference(sd, utts, pace)                           # asserts the distance from every half-integer
        mel, t_lengths, durations, pitch = model.infer(text, pace=pace)
        assert durations.dtype == torch.int32 and mel.grad_fn is None
        for b, u in enumerate(utts):
            assert durations[b, :u["N"]].tolist() == want[b].tolist(), (pace, b)
            assert not durations[b, u["N"]:].any() and int(t_lengths[b]) == int(want[b].sum())
        if pace == 1.0:
            first = [int(w.sum()) for w in want]
            assert min(first) >= 3 and any(0 < d < 75 for d in want[0].tolist())
            again = model(text, durations, pitch)
            assert torch.equal(again[0].detach().view(torch.int32), mel.view(torch.int32))
            assert torch.equal(again[1], t_lengths) and torch.equal(again[3].detach().view(torch.int32), pitch.view(torch.int32))
        else:
            print("FIGURE predictor infer: frames at pace 1 %s, at pace 2 %s" % (first, t_lengths.tolist()))
            assert all(0.3 * a <= b <= 0.7 * a for a, b in zip(first, t_lengths.tolist()))
    capped = model.infer(text, max_duration=2)[2]
    assert int(capped.max()) == 2


def test_infer_pitch_transform_changes_the_mel(native_lib):
    model, _ = _infer_model()
    utts = pc.small_batch()
    text, _, _ = _device_batch(utts)
    seen = []

    def shift(pitch, lengths):
        seen.append((tuple(pitch.shape), lengths.tolist()))
        return pitch + 0.5
    plain = model.infer(text)
    moved = model.infer(text, pitch_transform=shift)
    assert seen == [((3, 12), list(pc.TOKENS))]
    assert torch.equal(plain[2], moved[2]) and torch.equal(moved[3], plain[3] + 0.5)
    assert float((plain[0] - moved[0]).abs().max()) > 1e-3


def test_no_host_copies_with_device_lengths_and_max_frames(native_lib):
    from tacotron2_amd import fastpitch
    model, _ = _infer_model()
    utts = pc.small_batch()
    text, dur, pitch = _device_batch(utts, nan_pitch=False)
    n_dev = torch.tensor(pc.TOKENS, dtype=torch.int32, device=DEV)
    target = torch.randn(3, 16, 80, device=DEV)
    loss = fastpitch.FastPitchLoss()

    def step():
        out = model(text, dur, pitch, text_lengths=n_dev, max_frames=14)
        loss(out, target, dur, pitch, None, n_dev)[0].backward()
        return model.infer(text, text_lengths=n_dev, max_frames=60)
    step()                                                                  # warm: the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        mel = step()[0]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert tuple(mel.shape) == (3, 60, 80)


def test_twenty_adam_steps_reduce_the_loss(native_lib):
    from tacotron2_amd import fastpitch
    model, _ = pc.small_model()
    model = model.to(DEV)
    utts = pc.small_batch()
    text, dur, pitch = _device_batch(utts, nan_pitch=False)
    n_dev = torch.tensor(pc.TOKENS, dtype=torch.int32, device=DEV)
    T = max(u["T"] for u in utts)
    target = pc.layout([u["mel"] for u in utts], DEV, T)
    loss, opt = fastpitch.FastPitchLoss(), torch.optim.Adam(model.parameters(), lr=1e-3)
    values = []
    for _ in range(21):
        opt.zero_grad()
        total, _ = loss(model(text, dur, pitch, text_lengths=n_dev, max_frames=T), target, dur, pitch, None, n_dev)
        values.append(total.detach())
        total.backward()
        opt.step()
    first, last = float(values[0]), float(values[-1])
    print("FIGURE predictor training: FastPitchLoss %.6f before and %.6f after 20 Adam steps" % (first, last))
    assert math.isfinite(last) and last < first


def test_bench_tool_smallest_case(native_lib):
    import json
    import os
    import subprocess
    import sys
    import golden_util as gu
    out = subprocess.run([sys.executable, os.path.join(gu.ROOT, "tools", "bench_fastpitch.py"), "--smallest", "--iters", "2"],
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["cases"] and all(c["project_native_fwd_ms"] > 0 and c["model_torch_fwd_bwd_ms"] > 0 and c["infer_native_ms"] > 0
                                for c in res["cases"])
