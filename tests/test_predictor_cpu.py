"""The thin projection and the thin embedding of a temporal predictor, the predictor, FastPitch and its loss without a GPU: the
float64 definition (tests/predictor_ref.py) against float64 torch run on each utterance alone and against a padded batch (which
differs), the float32 restatement against the float64 one, csrc/predictor_rows.hip itself run on the host stand-in bit for bit
against the restatement, the refusals, the C entries' argument checks, the modules' state dicts and the loss against a loop."""
import contextlib
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import predictor_cases as pc
import predictor_ref as pr
from tacotron2_amd import fastpitch, native

CPU = torch.device("cpu")
F32 = np.float32


# ---- the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 4])
def test_float64_projection_equals_torch_linear_on_each_utterance_alone(P):
    batch = pc.project_batch((1, 3, 9), 36, P, True, seed=P)
    w, b = torch.from_numpy(batch["w"]).double().requires_grad_(True), torch.from_numpy(batch["b"]).double().requires_grad_(True)
    for u in batch["utts"]:
        h = torch.from_numpy(u["h"]).double().requires_grad_(True)
        y = F.linear(h, w, b)
        dh, dw, db = torch.autograd.grad(y, (h, w, b), torch.from_numpy(u["g"]).double())
        for name, got in (("y", y.detach()), ("dh", dh), ("dw", dw), ("db", db)):
            assert np.abs(got.numpy() - u["f64"][name]).max() <= 1e-12 * max(1.0, np.abs(u["f64"][name]).max()), (u["T"], name)


@pytest.mark.parametrize("shape", [(32, 1, 3), (36, 2, 9), (64, 4, 1), (32, 3, 5)])
def test_float64_embedding_equals_torch_conv1d_on_each_utterance_alone(shape):
    """Every T_b from 1 to 9: forward and the autograd gradients of F.conv1d on the tracks trimmed to T_b, plus the base."""
    C, P, k = shape
    batch = pc.embed_batch(tuple(range(1, 10)), C, P, k, True, True, seed=k)
    w, b = torch.from_numpy(batch["w"]).double().requires_grad_(True), torch.from_numpy(batch["b"]).double().requires_grad_(True)
    for u in batch["utts"]:
        v = torch.from_numpy(u["v"]).double().requires_grad_(True)
        base = torch.from_numpy(u["base"]).double().requires_grad_(True)
        y = base + F.conv1d(v.t()[None], w, b, padding=k // 2)[0].t()
        dv, dw, db, dbase = torch.autograd.grad(y, (v, w, b, base), torch.from_numpy(u["g"]).double())
        for name, got in (("y", y.detach()), ("dv", dv), ("dw", dw), ("db", db), ("dbase", dbase)):
            assert np.abs(got.numpy() - u["f64"][name]).max() <= 1e-12 * max(1.0, np.abs(u["f64"][name]).max()), (u["T"], name)


@pytest.mark.parametrize("k", [3, 9])
def test_a_padded_batch_embedding_differs_in_the_last_frames(k):
    """nn.Conv1d over a padded batch whose padding holds the track's fill value (the align tool writes 0 Hz there, a normalised
    track holds -mean / std): the last k // 2 frames read it and differ from the utterance alone; every earlier frame agrees."""
    r = np.random.default_rng(k)
    w = r.standard_normal((32, 1, k)).astype(F32)
    b = r.standard_normal(32).astype(F32)
    T, Tm = 12, 20
    v = r.standard_normal((T, 1)).astype(F32)
    alone = pr.embed64(v, w, b, None)
    vp = torch.full((Tm,), -1.5, dtype=torch.float64)
    vp[:T] = torch.from_numpy(v[:, 0]).double()
    padded = F.conv1d(vp[None, None], torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=k // 2)[0].t().numpy()
    assert np.abs(padded[:T - k // 2] - alone[:T - k // 2]).max() <= 1e-12
    for t in range(T - k // 2, T):
        assert np.abs(padded[t] - alone[t]).max() > 1e-3, t


def test_float32_restatement_is_close_to_float64():
    """C terms behind a projection, P k behind an embedding, B T behind a sum: 8 n u max(1, |value|) bounds the error with room."""
    batch = pc.project_batch((1, 5, 40), 384, 4, True)
    for u in batch["utts"]:
        assert pr.error(u["f32"]["y"], u["f64"]["y"]) <= 8 * 384 * pr.U * max(1.0, np.abs(u["f64"]["y"]).max())
        assert pr.error(u["f32"]["dh"], u["f64"]["dh"]) <= 8 * 4 * pr.U * max(1.0, np.abs(u["f64"]["dh"]).max())
    f64, f32 = pc.project_batch_sums(batch, 40)
    for n in ("dw", "db"):
        assert pr.error(f32[n], f64[n]) <= 8 * 46 * pr.U * max(1.0, np.abs(f64[n]).max()), n
    batch = pc.embed_batch((1, 5, 40), 36, 2, 9, True, True)
    for u in batch["utts"]:
        assert pr.error(u["f32"]["y"], u["f64"]["y"]) <= 8 * 20 * pr.U * max(1.0, np.abs(u["f64"]["y"]).max())
        assert pr.error(u["f32"]["dv"], u["f64"]["dv"]) <= 8 * 9 * 36 * pr.U * max(1.0, np.abs(u["f64"]["dv"]).max())
    f64, f32 = pc.embed_batch_sums(batch, 40)
    for n in ("dw", "db"):
        assert pr.error(f32[n], f64[n]) <= 8 * 46 * pr.U * max(1.0, np.abs(f64[n]).max()), n


# ---- csrc/predictor_rows.hip on the host stand-in ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("build_predictor_emu", os.path.join(gu.ROOT, "tests", "hip_emu", "build_predictor_emu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(mod.build(str(tmp_path_factory.mktemp("predictor_emu"))))
    assert lib.t2amd_emulated() == 1
    for name, at in native._argtypes().items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = at, ctypes.c_int
    lib.t2amd_last_error.restype = ctypes.c_char_p
    return lib


@contextlib.contextmanager
def _emulated(lib):
    saved = (native._lib, native._validate_only)
    native._lib, native._validate_only = lib, True            # CPU pointers allowed, kernels DO run (emulated)
    try:
        yield
    finally:
        native._lib, native._validate_only = saved


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("P", [1, 2, 4])
@pytest.mark.parametrize("C", [32, 36, 384, 1028])
def test_emulated_projection_equals_the_restatement_bit_for_bit(emu, C, P, bias):
    """y, dh, dw and db through the autograd function, on a ragged batch with NaN in the padding; the outputs are torch.empty
    tensors the kernels must write in full (the padding is checked for +0 bits)."""
    batch = pc.project_batch((0, 1, 3, 65), C, P, bias)
    with _emulated(emu):
        out = pc.run_project(batch, CPU, T=67, offset=1, device_lengths=False)
        pc.check_project(batch, out, "emulated ", exact=True)
        again = pc.run_project(batch, CPU, T=67, offset=0, device_lengths=False)
        for n in out:
            if n != "T":
                assert np.array_equal(pc.bits(out[n]), pc.bits(again[n])), n


@pytest.mark.parametrize("base", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", pc.EMBED_SHAPES + ((1028, 3, 5),))
def test_emulated_embedding_equals_the_restatement_bit_for_bit(emu, shape, bias, base):
    """Utterances of up to 9 frames in three workgroups of four rows: at k = 9 every tap lies outside the utterance at some frame.
    (The stand-in synchronises 256 host threads at every wave sum, of which dv takes P k a row: longer batches run on the GPU.)"""
    batch = pc.embed_batch((0, 1, 2, 4, 5, 9), *shape, bias, base)
    with _emulated(emu):
        out = pc.run_embed(batch, CPU, T=11, offset=1, device_lengths=False)
        pc.check_embed(batch, out, "emulated ", exact=True)
        again = pc.run_embed(batch, CPU, T=10, offset=0, device_lengths=False)
        for n in ("y", "dv", "dbase"):
            if n in out:
                assert np.array_equal(pc.bits(out[n][:, :9]), pc.bits(again[n][:, :9])), n


def test_emulated_entries_write_poisoned_outputs_in_full(emu):
    """Every output of every entry starts as 7.0 and ends as the restatement on the real rows and +0 bits beyond; the sums over
    many short utterances take more than one partial sum; limits and workspaces."""
    Ts = tuple(1 + i % 7 for i in range(40))
    T, C, P, k = 7, 36, 2, 3
    B = len(Ts)
    parts, RP = pr.sum_plan(B, T)
    assert parts == 5
    proj, emb = pc.project_batch(Ts, C, P, True), pc.embed_batch(Ts, C, P, k, True, True)
    lens = torch.tensor(Ts, dtype=torch.int32)
    seven = lambda *s: torch.full(s, 7.0)                                   # noqa: E731
    with _emulated(emu):
        h, g = (pc.layout([u[n] for u in proj["utts"]], CPU, T).contiguous() for n in ("h", "g"))
        w, b = torch.from_numpy(proj["w"]), torch.from_numpy(proj["b"])
        y, dh, dw, db = seven(B, T, P), seven(B, T, C), seven(P, C), seven(P)
        native.pred_project(h, w, b, lens, y)
        native.pred_project_backward(g, w, lens, dh)
        ws = torch.zeros(native.predictor_workspace(B, T, C, P, 1, 1), dtype=torch.uint8)
        native.pred_project_sums(g, h, lens, dw, db, ws)
        pc.check_project(proj, dict(y=y.numpy(), dh=dh.numpy(), dw=dw.numpy(), db=db.numpy(), T=T), "poisoned ", exact=True)
        v, ge, base = (pc.layout([u[n] for u in emb["utts"]], CPU, T).contiguous() for n in ("v", "g", "base"))
        image = torch.from_numpy(np.ascontiguousarray(emb["w"].transpose(1, 2, 0)).reshape(P * k, C))
        ye, dbase, dv, dwe, dbe = seven(B, T, C), seven(B, T, C), seven(B, T, P), seven(C, P, k), seven(C)
        native.pred_embed(v, image, torch.from_numpy(emb["b"]), base, lens, k, ye)
        native.pred_embed_backward(ge, image, lens, P, k, dbase, dv)
        wse = torch.zeros(native.predictor_workspace(B, T, C, P, k, 2), dtype=torch.uint8)
        native.pred_embed_sums(ge, v, lens, k, dwe, dbe, wse)
        pc.check_embed(emb, dict(y=ye.numpy(), dbase=dbase.numpy(), dv=dv.numpy(), dw=dwe.numpy(), db=dbe.numpy(), T=T), "poisoned ",
                       exact=True)
        only = seven(B, T, C)
        native.pred_embed_backward(ge, None, lens, P, k, only, None)       # dbase alone needs no image
        assert torch.equal(only.view(torch.int32), dbase.view(torch.int32))
        assert native.predictor_limits() == (4096, 4096, 9, 4, 65535)
        assert native.predictor_workspace(B, T, C, P, k, 0) == 0
        assert native.predictor_workspace(B, T, C, P, k, 1) == 4 * parts * (P * C + 4)
        assert native.predictor_workspace(B, T, C, P, k, 2) == 4 * parts * (P * k + 1) * C


def test_emulated_public_functions_keep_nothing_under_no_grad_and_take_one_track_as_a_matrix(emu):
    batch = pc.embed_batch((2, 5), 32, 1, 3, True, True)
    with _emulated(emu):
        v = pc.layout([u["v"] for u in batch["utts"]], CPU, 6)
        base = pc.layout([u["base"] for u in batch["utts"]], CPU, 6).requires_grad_(True)
        w, b = torch.from_numpy(batch["w"]).requires_grad_(True), torch.from_numpy(batch["b"])
        y3 = fastpitch.scalar_embed(v, w, b, [2, 5], base)
        y2 = fastpitch.scalar_embed(v[:, :, 0], w, b, [2, 5], base)
        assert y3.grad_fn is not None and torch.equal(y3.detach().view(torch.int32), y2.detach().view(torch.int32))
        y3.backward(pc.layout([u["g"] for u in batch["utts"]], CPU, 6))
        assert base.grad is not None and w.grad is not None and not base.grad[0, 2:].view(torch.int32).any()
        with torch.no_grad():
            assert fastpitch.scalar_embed(v, w, b, [2, 5], base).grad_fn is None
            assert fastpitch.channel_project(base, torch.zeros(2, 32).requires_grad_(True), None, [2, 5]).grad_fn is None
        pred = fastpitch.TemporalPredictor(32, 32, 3, n_predictions=2)
        # the ragged convolution is an MFMA kernel, which the host stand-in does not have: only the thin end is run here
        assert tuple(fastpitch.channel_project(base, pred.fc.weight, pred.fc.bias, [2, 5]).shape) == (2, 6, 2)


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(emu):
    proj, emb = fastpitch.channel_project, fastpitch.scalar_embed
    with _emulated(emu):                                                    # host tensors pass the device check here
        h, w, b = torch.zeros(2, 6, 32), torch.zeros(2, 32), torch.zeros(2)
        with pytest.raises(TypeError, match="channel_project: expected float32 h"):
            proj(h.double(), w, b)
        with pytest.raises(TypeError, match="channel_project: expected float32 weight"):
            proj(h, w.half(), b)
        with pytest.raises(TypeError, match="channel_project: expected float32 bias"):
            proj(h, w, b.double())
        with pytest.raises(ValueError, match=r"channel_project: expected h \(B, T, C\)"):
            proj(h[0], w, b)
        with pytest.raises(ValueError, match=r"channel_project: expected weight \(P, 32\)"):
            proj(h, torch.zeros(2, 64), b)
        with pytest.raises(ValueError, match=r"channel_project: 5 values per row do not lie in \[1, 4\]"):
            proj(h, torch.zeros(5, 32))
        with pytest.raises(ValueError, match="channel_project: expected bias"):
            proj(h, w, torch.zeros(3))
        for C in (16, 34, 4100):
            with pytest.raises(ValueError, match="channel_project: %d channels are not a multiple of 4 from 32 to 4096" % C):
                proj(torch.zeros(1, 2, C), torch.zeros(1, C))
        with pytest.raises(ValueError, match="channel_project: 4097 frames exceed the limit of 4096"):
            proj(torch.zeros(1, 4097, 32), w)
        with pytest.raises(ValueError, match=r"channel_project: utterance 1: 7 frames do not lie in \[0, 6\]"):
            proj(h, w, b, [6, 7])
        v, we, be = torch.zeros(2, 6), torch.zeros(32, 1, 3), torch.zeros(32)
        with pytest.raises(TypeError, match="scalar_embed: expected float32 v"):
            emb(v.long(), we, be)
        with pytest.raises(TypeError, match="scalar_embed: expected float32 weight"):
            emb(v, we.double(), be)
        with pytest.raises(TypeError, match="scalar_embed: expected float32 base"):
            emb(v, we, be, None, torch.zeros(2, 6, 32).double())
        with pytest.raises(ValueError, match=r"scalar_embed: expected v \(B, T\) or \(B, T, P\)"):
            emb(torch.zeros(6), we, be)
        with pytest.raises(ValueError, match="scalar_embed: 5 scalar tracks exceed the limit of 4"):
            emb(torch.zeros(2, 6, 5), torch.zeros(32, 5, 3))
        with pytest.raises(ValueError, match=r"scalar_embed: expected weight \(C, 1, k\)"):
            emb(v, torch.zeros(32, 2, 3), be)
        for k in (2, 11):
            with pytest.raises(ValueError, match="scalar_embed: a kernel width of %d is not odd and at most 9" % k):
                emb(v, torch.zeros(32, 1, k))
        with pytest.raises(ValueError, match="scalar_embed: 30 channels are not a multiple of 4 from 32 to 4096"):
            emb(v, torch.zeros(30, 1, 3))
        with pytest.raises(ValueError, match="scalar_embed: expected bias"):
            emb(v, we, torch.zeros(31))
        with pytest.raises(ValueError, match="scalar_embed: expected base"):
            emb(v, we, be, None, torch.zeros(2, 5, 32))
        with pytest.raises(ValueError, match="scalar_embed: 1 lengths for a batch of 2"):
            emb(v, we, be, [6])
    with pytest.raises(native.NativeError, match="channel_project: h is on cpu.*no CPU path"):
        proj(torch.zeros(1, 4, 32), torch.zeros(1, 32))
    with pytest.raises(native.NativeError, match="scalar_embed: v is on cpu.*no CPU path"):
        emb(torch.zeros(1, 4), torch.zeros(32, 1, 3))
    with pytest.raises(native.NativeError, match="no CPU path"):
        fastpitch.TemporalPredictor(32, 32, 3)(torch.zeros(1, 4, 32))


def test_modules_state_dicts_and_construction_refusals():
    tp = fastpitch.TemporalPredictor(64, 32, 5, n_layers=3, n_predictions=2)
    assert sorted(tp.state_dict()) == sorted(["layers.%d.%s.%s" % (i, m, p) for i in range(3) for m in ("conv", "norm") for p in ("weight", "bias")]
                                             + ["fc.weight", "fc.bias"])
    assert tuple(tp.layers[0].conv.weight.shape) == (32, 64, 5) and tuple(tp.layers[2].conv.weight.shape) == (32, 32, 5)
    assert tuple(tp.fc.weight.shape) == (2, 32)
    for args, word in (((48, 32, 3), "input_size must be a multiple of 32"), ((32, 4128, 3), "filter_size must be a multiple of 32"),
                       ((32, 32, 4), "kernel_size must be an odd int up to 9"), ((32, 32, 11), "kernel_size must be an odd int"),
                       ((32, 32, 3, 0), "n_layers must be an int of at least 1"), ((32, 32, 3, 2, 5), "5 predictions exceed the limit of 4"),
                       ((32, 32, 3, 2, True), "n_predictions must be an int")):
        with pytest.raises(ValueError, match="TemporalPredictor: " + word):
            fastpitch.TemporalPredictor(*args)
    with pytest.raises(ValueError, match=r"TemporalPredictor: expected x \(B, T, 64\)"):
        tp(torch.zeros(2, 5, 32))
    model = fastpitch.FastPitch(**pc.SMALL)
    sd = model.state_dict()
    for key in ("encoder.word_emb.weight", "encoder.layers.1.pos_ff.conv2.weight", "decoder.layers.0.dec_attn.qkv_net.weight",
                "duration_predictor.layers.1.norm.bias", "duration_predictor.fc.weight", "pitch_predictor.layers.0.conv.weight",
                "pitch_emb.weight", "pitch_emb.bias", "proj.weight", "proj.bias"):
        assert key in sd, key
    assert not any(k.startswith("energy") for k in sd) and "decoder.word_emb.weight" not in sd
    assert tuple(sd["pitch_emb.weight"].shape) == (64, 1, 3) and tuple(sd["proj.weight"].shape) == (80, 64)
    assert tuple(sd["encoder.word_emb.weight"].shape) == (11, 64) and tuple(sd["duration_predictor.fc.weight"].shape) == (1, 64)
    with_energy = fastpitch.FastPitch(**dict(pc.SMALL, energy_conditioning=True)).state_dict()
    assert "energy_emb.weight" in with_energy and "energy_predictor.fc.bias" in with_energy
    full = fastpitch.FastPitch(148)
    assert tuple(full.pitch_emb.weight.shape) == (384, 1, 3) and len(full.encoder.layers) == 6 and tuple(full.proj.weight.shape) == (80, 384)
    assert tuple(full.duration_predictor.layers[0].conv.weight.shape) == (256, 384, 3)
    for kw, word in ((dict(d_model=48), "d_model must be a multiple of 32, at most 512"), (dict(d_model=1024), "d_model must be"),
                     (dict(n_mel=30), "n_mel must be a multiple of 4 from 32"), (dict(pitch_kernel=4), "pitch_kernel must be an odd int"),
                     (dict(n_symbols=1), "n_symbols must be an int of at least 2"), (dict(padding_idx=11), "padding_idx must be an int in")):
        with pytest.raises(ValueError, match="FastPitch: " + word):
            fastpitch.FastPitch(**dict(pc.SMALL, **kw))
    text = torch.ones(2, 5, dtype=torch.long)
    with pytest.raises(ValueError, match=r"FastPitch: expected integer symbols \(B, N\)"):
        model(torch.zeros(2, 5), torch.ones(2, 5, dtype=torch.int32), torch.zeros(2, 5))
    with pytest.raises(TypeError, match="FastPitch: expected float32 pitch"):
        model(text, torch.ones(2, 5, dtype=torch.int32), torch.zeros(2, 5).double())
    with pytest.raises(ValueError, match=r"FastPitch: expected pitch of shape \(2, 5\)"):
        model(text, torch.ones(2, 5, dtype=torch.int32), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="FastPitch: energy targets were given to a model without energy conditioning"):
        model(text, torch.ones(2, 5, dtype=torch.int32), torch.zeros(2, 5), torch.zeros(2, 5))
    with pytest.raises(native.NativeError, match="no CPU path"):
        model(text, torch.ones(2, 5, dtype=torch.int32), torch.zeros(2, 5))
    with pytest.raises(ValueError, match="FastPitch.infer: the pace must be a positive number"):
        model.infer(text, pace=0.0)
    with pytest.raises(ValueError, match="FastPitchLoss: dur_scale must be a finite number"):
        fastpitch.FastPitchLoss(dur_scale=-1.0)


def test_fastpitch_host_plumbing_validate_only(native_lib, monkeypatch):
    """forward + backward and infer with every kernel skipped: the shapes, the launch arguments and the C checks of the whole
    path, without a GPU.  No kernel writes the regulator's frame counts here, and a host tensor of lengths is read and checked,
    so the test fills them in."""
    real = native.durations_to_path

    def with_frame_counts(durations, n_len, T, path, t_lengths, *rest):
        real(durations, n_len, T, path, t_lengths, *rest)
        t_lengths.fill_(T)
    monkeypatch.setattr(native, "durations_to_path", with_frame_counts)
    native.set_validate_only(True)
    try:
        model = fastpitch.FastPitch(**dict(pc.SMALL, energy_conditioning=True))
        utts = pc.small_batch()
        text = pc.pad_tokens(utts, "ids", CPU, torch.long)
        dur = pc.pad_tokens(utts, "durations", CPU, torch.int32)
        pitch = pc.pad_tokens(utts, "pitch", CPU, torch.float32)
        out = model(text, dur, pitch, energy=pitch.clone(), text_lengths=list(pc.TOKENS), max_frames=40)
        assert tuple(out[0].shape) == (3, 40, 80) and tuple(out[2].shape) == (3, 12) and tuple(out[4].shape) == (3, 12)
        total, parts = fastpitch.FastPitchLoss()(out, torch.zeros(3, 44, 80), dur, pitch, pitch, torch.tensor(pc.TOKENS))
        total.backward()
        assert all(p.grad is not None and p.grad.shape == p.shape for p in model.parameters())
        assert sorted(parts) == ["duration", "energy", "mel", "pitch"]
        mel, t_lengths, durations, p = model.infer(text, max_frames=30, pitch_transform=lambda x, n: x + 1.0)
        assert tuple(mel.shape) == (3, 30, 80) and durations.dtype == torch.int32 and tuple(p.shape) == (3, 12) and mel.grad_fn is None
    finally:
        native.set_validate_only(False)


def test_fastpitch_loss_equals_a_float64_loop():
    """Random outputs with NaN beyond every length in the predictions and the targets."""
    r = np.random.default_rng(5)
    Ts, Ns, T, N, M = (4, 0, 9), (3, 1, 5), 9, 6, 32
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64)       # noqa: E731
    mel_out, mel, log_dur, pitch_pred, pitch, e_pred, e_tgt = nan(3, T, M), nan(3, T + 2, M), nan(3, N), nan(3, N), nan(3, N), nan(3, N), nan(3, N)
    dur = torch.full((3, N), -3, dtype=torch.int64)
    per = dict(mel_out=[], mel=[], log_dur=[], dur=[], pitch_pred=[], pitch=[], e_pred=[], e_tgt=[])
    for b, (t, n) in enumerate(zip(Ts, Ns)):
        for name, tensor, shape in (("mel_out", mel_out, (t, M)), ("mel", mel, (t, M)), ("log_dur", log_dur, (n,)), ("pitch_pred", pitch_pred, (n,)),
                                    ("pitch", pitch, (n,)), ("e_pred", e_pred, (n,)), ("e_tgt", e_tgt, (n,))):
            a = r.standard_normal(shape)
            per[name].append(a)
            tensor[b, :shape[0]] = torch.from_numpy(a)
        d = r.integers(0, 5, (n,))
        per["dur"].append(d)
        dur[b, :n] = torch.from_numpy(d)
    t_len, n_len = torch.tensor(Ts, dtype=torch.int32), torch.tensor(Ns, dtype=torch.int32)
    loss = fastpitch.FastPitchLoss(0.1, 0.2, 0.3)
    total, parts = loss((mel_out, t_len, log_dur, pitch_pred, e_pred), mel, dur, pitch, e_tgt, n_len)
    want, want_parts = pc.loss_ref(per["mel_out"], per["mel"], per["log_dur"], per["dur"], per["pitch_pred"], per["pitch"], (0.1, 0.2),
                                   (per["e_pred"], per["e_tgt"], 0.3))
    assert abs(float(total) - want) <= 1e-12 * abs(want)
    for n in want_parts:
        assert abs(float(parts[n]) - want_parts[n]) <= 1e-12 * abs(want_parts[n]), n
    total2, parts2 = loss((mel_out[:, :, :], t_len, log_dur, pitch_pred, None), mel, dur, pitch, None, n_len)
    assert sorted(parts2) == ["duration", "mel", "pitch"] and float(total2) < float(total)
    with pytest.raises(ValueError, match="FastPitchLoss: expected a target mel"):
        loss((mel_out, t_len, log_dur, pitch_pred, None), mel[:, :T - 1], dur, pitch, None, n_len)
    with pytest.raises(ValueError, match="FastPitchLoss: energy targets and an energy prediction"):
        loss((mel_out, t_len, log_dur, pitch_pred, None), mel, dur, pitch, e_tgt, n_len)


# ---- the C entries' own checks -------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments(emu):
    hold = torch.zeros(1 << 18)                                             # the accepted calls run their kernels in here
    try:
        base = hold.data_ptr() // 16 * 16 + 16
        at = lambda i: ctypes.c_void_p(base + i * (1 << 15))                # noqa: E731
        h, w, b, y, g, dh, ws, v, img, e = (at(i) for i in range(10))
        off = lambda p: ctypes.c_void_p(p.value + 4)                        # noqa: E731
        n = ctypes.c_longlong(0)
        five = [ctypes.c_int(0) for _ in range(5)]
        assert emu.t2amd_predictor_limits(*[ctypes.byref(x) for x in five]) == 0 and [x.value for x in five] == [4096, 4096, 9, 4, 65535]
        assert emu.t2amd_predictor_limits(None, None, None, None, None) != 0 and b"predictor: limits: null operand" in emu.t2amd_last_error()
        for args, word in (((1, 4, 32, 1, 3, 3), b"predictor: workspace: which must be"), ((0, 4, 32, 1, 3, 0), b"at least 1 utterance"),
                           ((1, 4097, 32, 1, 3, 1), b"at most 4096 frames"), ((65536, 4, 32, 1, 3, 0), b"at most 65535 utterances"),
                           ((1, 4, 32, 1, 4, 2), b"an odd kernel width from 1 to 9"), ((1, 4, 32, 1, 11, 2), b"an odd kernel width"),
                           ((1, 4, 30, 1, 3, 0), b"channels must be a multiple of 4, from 32 to 4096"), ((1, 4, 16, 1, 3, 0), b"from 32 to 4096"),
                           ((1, 4, 4100, 1, 3, 0), b"from 32 to 4096"), ((1, 4, 32, 0, 3, 0), b"1 to 4 scalar tracks"),
                           ((1, 4, 32, 5, 3, 0), b"1 to 4 scalar tracks")):
            assert emu.t2amd_predictor_workspace(*args, ctypes.byref(n)) != 0 and word in emu.t2amd_last_error(), word
        assert emu.t2amd_predictor_workspace(1, 4, 32, 1, 3, 0, None) != 0 and b"null operand" in emu.t2amd_last_error()
        names = ("h", "w", "bias", "len", "B", "T", "C", "P", "y", "stream")
        ok = (h, w, b, None, 2, 4, 32, 2, y, None)
        proj = lambda **kw: emu.t2amd_pred_project_f32(*[kw.get(nm, d) for nm, d in zip(names, ok)])       # noqa: E731
        assert proj() == 0 and proj(bias=None) == 0
        for kw, word in ((dict(h=None), b"predictor: project: null operand"), (dict(y=None), b"null operand"), (dict(P=5), b"1 to 4 scalar tracks"),
                         (dict(C=34), b"channels must be"), (dict(h=off(h)), b"aligned to 16 bytes"), (dict(w=off(w)), b"aligned to 16 bytes"),
                         (dict(y=h), b"must not overlap"), (dict(y=w), b"must not overlap"), (dict(y=b), b"must not overlap")):
            assert proj(**kw) != 0 and word in emu.t2amd_last_error(), word
        assert emu.t2amd_pred_project_bwd_f32(g, w, None, 2, 4, 32, 2, dh, None) == 0
        for args, word in (((None, w, None, 2, 4, 32, 2, dh, None), b"predictor: project_bwd: null operand"),
                           ((g, w, None, 2, 4, 32, 2, off(dh), None), b"aligned to 16 bytes"), ((g, w, None, 2, 4, 32, 2, w, None), b"must not overlap"),
                           ((g, w, None, 2, 4, 32, 2, g, None), b"must not overlap"), ((g, w, None, 2, 4097, 32, 2, dh, None), b"at most 4096 frames")):
            assert emu.t2amd_pred_project_bwd_f32(*args) != 0 and word in emu.t2amd_last_error(), word
        need = 4 * (2 * 32 + 4)
        assert emu.t2amd_pred_project_sums_f32(g, h, None, 2, 4, 32, 2, y, b, ws, need, None) == 0
        assert emu.t2amd_pred_project_sums_f32(g, h, None, 2, 4, 32, 2, None, b, ws, need, None) == 0
        for args, word in (((g, h, None, 2, 4, 32, 2, None, None, ws, need, None), b"predictor: project_sums: null operand"),
                           ((g, h, None, 2, 4, 32, 2, y, b, ws, need - 1, None), b"workspace is smaller"),
                           ((g, h, None, 2, 4, 32, 2, y, b, off(ws), need, None), b"not aligned to 16 bytes"),
                           ((g, h, None, 2, 4, 32, 2, y, b, h, need, None), b"must not overlap"),
                           ((g, h, None, 2, 4, 32, 2, y, y, ws, need, None), b"must not overlap"),
                           ((g, h, None, 2, 4, 32, 2, g, b, ws, need, None), b"must not overlap")):
            assert emu.t2amd_pred_project_sums_f32(*args) != 0 and word in emu.t2amd_last_error(), word
        enames = ("v", "img", "bias", "base", "len", "B", "T", "C", "P", "k", "y", "stream")
        eok = (v, img, b, h, None, 2, 4, 32, 2, 3, e, None)
        emb = lambda **kw: emu.t2amd_pred_embed_f32(*[kw.get(nm, d) for nm, d in zip(enames, eok)])        # noqa: E731
        assert emb() == 0 and emb(bias=None, base=None) == 0
        for kw, word in ((dict(v=None), b"predictor: embed: null operand"), (dict(img=None), b"null operand"), (dict(k=2), b"an odd kernel width"),
                         (dict(P=0), b"1 to 4 scalar tracks"), (dict(base=off(h)), b"aligned to 16 bytes"), (dict(y=off(e)), b"aligned to 16 bytes"),
                         (dict(y=h), b"must not overlap"), (dict(y=v), b"must not overlap"), (dict(y=img), b"must not overlap")):
            assert emb(**kw) != 0 and word in emu.t2amd_last_error(), word
        assert emu.t2amd_pred_embed_bwd_f32(e, img, None, 2, 4, 32, 2, 3, dh, g, None) == 0
        assert emu.t2amd_pred_embed_bwd_f32(e, None, None, 2, 4, 32, 2, 3, dh, None, None) == 0
        for args, word in (((e, img, None, 2, 4, 32, 2, 3, None, None, None), b"predictor: embed_bwd: null operand"),
                           ((e, None, None, 2, 4, 32, 2, 3, dh, g, None), b"null operand"), ((e, img, None, 2, 4, 32, 2, 3, e, g, None), b"must not overlap"),
                           ((e, img, None, 2, 4, 32, 2, 3, dh, img, None), b"must not overlap"), ((off(e), img, None, 2, 4, 32, 2, 3, dh, g, None), b"aligned to 16")):
            assert emu.t2amd_pred_embed_bwd_f32(*args) != 0 and word in emu.t2amd_last_error(), word
        need = 4 * (2 * 3 + 1) * 32
        assert emu.t2amd_pred_embed_sums_f32(e, v, None, 2, 4, 32, 2, 3, y, b, ws, need, None) == 0
        for args, word in (((e, v, None, 2, 4, 32, 2, 3, None, None, ws, need, None), b"predictor: embed_sums: null operand"),
                           ((e, v, None, 2, 4, 32, 2, 3, y, b, ws, need - 1, None), b"workspace is smaller"),
                           ((e, v, None, 2, 4, 32, 2, 3, y, b, e, need, None), b"must not overlap"),
                           ((e, v, None, 2, 4, 32, 2, 3, v, b, ws, need, None), b"must not overlap")):
            assert emu.t2amd_pred_embed_sums_f32(*args) != 0 and word in emu.t2amd_last_error(), word
    finally:
        del hold


# ---- the rows file under the address and undefined-behaviour sanitizers --------------------------------------------------------
def test_rows_kernels_run_clean_in_a_stand_alone_sanitizer_program(tmp_path):
    """csrc/predictor_rows.hip, the stand-in runtime and tests/hip_emu/predictor_sanitize_main.cpp (its own main: every kernel once
    on ragged batches with tensors of exactly the sizes the entries state) built by the host compiler with
    -fsanitize=address,undefined and run as a program of its own."""
    emu_dir = os.path.join(gu.ROOT, "tests", "hip_emu")
    exe = str(tmp_path / "predictor_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-pthread", "-I", emu_dir, "-x", "c++",
                           os.path.join(gu.ROOT, "tacotron2_amd", "csrc", "predictor_rows.hip"), os.path.join(emu_dir, "emu_runtime.cpp"),
                           os.path.join(emu_dir, "predictor_sanitize_main.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
