"""WaveGlow's forward direction without a GPU: the float64 restatement tests/waveglow_fwd_ref.py inverts
WaveGlowRef.infer, the latent / noise reorderings, the refusals of WaveGlow.forward and of the two new entry points
(validate-only), and csrc/waveglow_fwd.hip run on the host stand-in of tests/hip_emu -- the flow head and the loss
reduction directly against float64 numpy on a ragged batch with an early boundary, and the whole WaveGlow.forward /
nll / WaveGlowLoss with the products stood in by float64 torch (as tests/test_waveglow_cpu.py does for infer), full and
ragged, against the restatement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import golden_util as gu
import test_waveglow_cpu as base
import waveglow_fwd_ref as fr
import waveglow_ref as wr
from tacotron2_amd import native
from tacotron2_amd import waveglow as wgm

EMU = base.EMU
SMALL = base.SMALL


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_restatement_round_trip_float64_and_reorderings():
    m = wr.make_ref(C=64, L=4).double()
    g = torch.Generator().manual_seed(5)
    B, N = 2, 9
    mel = (-5 + 2 * torch.randn(B, 80, N, generator=g)).double()
    audio = (0.3 * torch.randn(B, 256 * N, generator=g)).double()
    with torch.no_grad():
        z, ls, ld = fr.forward(m, mel, audio)
        back = m.infer(mel, 1.0, fr.latents_to_noise(m, z))
    assert z.shape == (B, 8, 32 * N) and [t.shape[1] for t in ls] == [4] * 4 + [3] * 4 + [2] * 4
    rel = _rel(back, audio)
    ls_max = max(t.abs().max().item() for t in ls)
    print("round trip %.3g, max |log_s| %.3g, loss %.6f" % (rel, ls_max, fr.loss((z, ls, ld)).item()))
    assert rel < 1e-12
    assert ls_max > 1e-2
    # the reorderings, on the restatement and on the module
    wg = wgm.WaveGlow.from_module(m.float())
    noise = wg.latents_to_noise(z)
    assert [tuple(t.shape) for t in noise] == wg.noise_shapes(B, N)
    assert torch.equal(noise[0], z[:, 4:]) and torch.equal(noise[1], z[:, 2:4]) and torch.equal(noise[2], z[:, 0:2])
    assert torch.equal(wg.noise_to_latents(noise), z)
    assert all(torch.equal(a, b) for a, b in zip(noise, fr.latents_to_noise(m, z)))
    assert torch.equal(fr.noise_to_latents(m, noise), z)
    with pytest.raises(ValueError, match="expected 3"):
        wg.noise_to_latents(noise[:2])


def test_forward_plan_keeps_partial_frames_inside_the_utterance():
    wg = wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=3))
    H = wg.halo()
    rowb, rowr, offs, P = wg.forward_plan([40, 64, 3], [2, 2, 1])
    assert offs == [H, H + 64 + H, H + 2 * (64 + H)] and P == H + 2 * (64 + H) + 32 + H
    rowb, rowr = rowb.numpy(), rowr.numpy()
    for b, (R, nf) in enumerate(zip([40, 64, 3], [2, 2, 1])):
        assert (rowb[offs[b]:offs[b] + R] == b).all() and (rowr[offs[b]:offs[b] + R] == np.arange(R)).all()
        assert (rowb[offs[b] + R:offs[b] + 32 * nf + H] == -1).all()      # the partial frame's tail and the halo
    assert (rowb[:H] == -1).all() and (rowb >= 0).sum() == 107


def test_forward_refuses_bad_shapes(native_lib):
    wg = wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=3))
    mel = torch.zeros(2, 80, 3)
    with pytest.raises(native.NativeError, match="no CPU path"):
        wg((mel, torch.zeros(2, 768)))
    with pytest.raises(native.NativeError, match="no CPU path"):
        wgm.WaveGlowLoss()((torch.zeros(1, 8, 4), [], []))
    with base._validate_only():
        z, ls, ld = wg((mel, torch.zeros(2, 768)))
        assert z.shape == (2, 8, 96) and [tuple(t.shape) for t in ls] == [(2, 4, 96)] * 2 + [(2, 3, 96)] * 2
        assert len(ld) == 4 and all(t.shape == () and t.dtype == torch.float32 for t in ld)
        assert not z.requires_grad and not any(t.requires_grad for t in ls)
        wg((mel, torch.zeros(2, 520)))                                      # T < 256 N, a partial last frame
        assert wg.nll(mel, torch.zeros(2, 768), lengths=[768, 264]).shape == (2,)
        assert wgm.WaveGlowLoss(0.7)((z, ls, ld)).shape == ()
        with pytest.raises(ValueError, match="multiples of n_group"):
            wg((mel, torch.zeros(2, 700)))
        with pytest.raises(ValueError, match="multiples of n_group"):
            wg((mel, torch.zeros(2, 768)), lengths=[768, 100])
        with pytest.raises(ValueError, match=r"at most 256 \* N = 768"):
            wg((mel, torch.zeros(2, 776)))
        with pytest.raises(ValueError, match="do not fit"):
            wg((mel, torch.zeros(2, 768)), lengths=[768, 776])
        with pytest.raises(ValueError, match="mels"):
            wg((torch.zeros(2, 40, 3), torch.zeros(2, 768)))
        with pytest.raises(ValueError, match="audio"):
            wg((mel, torch.zeros(2, 1, 768)))
        with pytest.raises(ValueError, match="audio"):
            wg((mel, torch.zeros(3, 768)))
        with pytest.raises(ValueError, match="audio must be float32"):
            wg((mel, torch.zeros(2, 768, dtype=torch.int16)))
        with pytest.raises(ValueError, match="mels must be float32"):
            wg((mel.double(), torch.zeros(2, 768)))
        with pytest.raises(ValueError, match="log_s"):
            wgm.WaveGlowLoss()((z, [torch.zeros(2, 4, 95)], ld))


def test_new_entry_points_reject_bad_arguments(native_lib):
    P, C, G, B, R = 80, 64, 8, 2, 30
    skip, h = torch.zeros(P, C), torch.zeros(P, C)
    rowb = torch.zeros(P, dtype=torch.int32)
    audio = torch.zeros(P, G)
    z, ls = torch.zeros(B, G, R), torch.zeros(B, 4, R)
    wave = torch.zeros(B, G * R)
    end = dict(skip=skip, end_w=torch.zeros(8, C), end_b=torch.zeros(8), log_s=ls)
    nxt = dict(mix_w=torch.zeros(6, 6), start_w=torch.zeros(C, 3), start_b=torch.zeros(C), h=h)
    err = base._err
    with base._validate_only():
        native.wg_head(rowb, rowb, audio, G, B, R, wave=wave, mix_w=torch.zeros(8, 8), start_w=torch.zeros(C, 4),
                       start_b=torch.zeros(C), h=h)
        native.wg_head(rowb, rowb, audio, G, B, R, z=z, z_off=0, n_emit=2, **end, **nxt)
        native.wg_head(rowb, rowb, audio, G, B, R, z=z, z_off=0, n_emit=8, **end)
        native.wg_head(rowb, rowb, audio, G, B, R, z=torch.zeros(B, 20, R)[:, 4:12], z_off=2, n_emit=2, **end, **nxt)
        err(native.wg_head, rowb, rowb, audio, G, B, R, skip=skip, match="either a flow to close")
        err(native.wg_head, rowb, rowb, audio, G, B, R, wave=wave, **end, match="either a flow to close")
        err(native.wg_head, rowb, rowb, audio, 7, B, R, wave=wave, h=h, match="n_group")
        err(native.wg_head, rowb, rowb, torch.zeros(P, 4), G, B, R, wave=wave, h=h, match="audio rows")
        err(native.wg_head, rowb, rowb, audio, G, B, R, wave=torch.zeros(B, G * R - 8), h=h, match="waveform rows")
        err(native.wg_head, rowb, rowb, audio, G, B, R, wave=wave.double(), h=h, match="float32")
        err(native.wg_head, rowb, rowb, audio, G, B, R, wave=wave, h=h, match="writes every remaining channel")
        err(native.wg_head, rowb, rowb, audio, G, B, R, z=z, n_emit=3, **end, **nxt, match="n_emit")
        err(native.wg_head, rowb, rowb, audio, G, B, R, z=z, z_off=7, n_emit=2, **end, **nxt, match="leaves z's channels")
        err(native.wg_head, rowb, rowb, audio, G, B, R, n_emit=2, **end, **nxt, match="needs z")
        err(native.wg_head, rowb, rowb, audio, G, B, R, z=z, n_emit=8, **end, **nxt, match="at least 2 channels")
        err(native.wg_head, rowb, rowb, audio, G, B, R, z=z, n_emit=2, mix_w=torch.zeros(6, 6), **end,
            match=r"needs start_w")
        err(native.wg_head, rowb, rowb, audio, G, B, R, z=torch.zeros(B, G, R + 1), n_emit=2, **end, **nxt, match="z ")
        err(native.wg_head, rowb, rowb, audio, G, B, R, z=z, n_emit=2, skip=skip, end_w=torch.zeros(8, C),
            end_b=torch.zeros(8), log_s=torch.zeros(B, 3, R), **nxt, match="log_s")
        err(native.wg_head, rowb, rowb, audio, G, B, R, z=z, n_emit=2, skip=skip, end_w=torch.zeros(8, 600),
            end_b=torch.zeros(8), log_s=ls, **nxt, match="C must")
        err(native.wg_head, rowb, rowb, audio, G, B, R, z=z.permute(0, 2, 1), n_emit=2, **end, **nxt, match="contiguous rows")
        lib = native.load()
        p = native.ptr
        err(native._check, lib.t2amd_wg_head_f32(None, C, C, p(end['end_w']), p(end['end_b']), 8, p(ls), 4 * R, R, None, 0,
                                                  p(audio), G, None, 0, 0, 0, 0, p(nxt['mix_w']), p(nxt['start_w']),
                                                  p(nxt['start_b']), p(h), C, p(rowb, torch.int32), p(rowb, torch.int32), P,
                                                  G, B, R, None), "x", match="null operand")
        err(native._check, lib.t2amd_wg_head_f32(p(skip), C, C, p(end['end_w']), p(end['end_b']), 8, p(ls), 4 * R, R - 1,
                                                  None, 0, p(audio), G, None, 0, 0, 0, 0, p(nxt['mix_w']), p(nxt['start_w']),
                                                  p(nxt['start_b']), p(h), C, p(rowb, torch.int32), p(rowb, torch.int32), P,
                                                  G, B, R, None), "x", match="log_s strides")
        # the reduction
        chunk = native.wg_nll_chunk()
        assert chunk == 2048
        rows = torch.zeros(B, dtype=torch.int32)
        part, out = torch.zeros(B * 2, dtype=torch.float64), torch.zeros(B, 2, dtype=torch.float64)
        native.wg_nll(z, ls, rows, part, out)
        native.wg_nll(z, None, rows, part, out)
        err(native.wg_nll, z, torch.zeros(B, 4, R + 1), rows, part, out, match="beside z")
        err(native.wg_nll, z, ls, rows, part[:2], out, match="partials")
        err(native.wg_nll, z, ls, rows, part.float(), out, match="float64")
        err(native.wg_nll, z.double(), ls, rows, part, out, match="float32")
        err(native.wg_nll, z, ls, rows.long(), part, out, match="int32")
        err(native.wg_nll, z.permute(0, 2, 1), ls, rows, part, out, match="contiguous rows")
        err(native._check, lib.t2amd_wg_nll_f32(p(z), G * R, R, G, p(ls), 4 * R, R, 4, p(rows, torch.int32), B, R,
                                                 p(part, torch.float64), 2, p(out, torch.float64), None), "x",
            match="partial needs")
        err(native._check, lib.t2amd_wg_nll_f32(p(z), G * R, R, G, None, 0, 0, 4, p(rows, torch.int32), B, R,
                                                 p(part, torch.float64), 1, p(out, torch.float64), None), "x",
            match="null operand")


# ---------------------------------------------------------------------------------------------------------------
# csrc/waveglow_fwd.hip (and csrc/waveglow.hip, for the round trip) on the host stand-in
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forward_emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("waveglow_fwd_emu") / "libwaveglow_fwd_emu.so")
    csrc = os.path.join(gu.ROOT, "tacotron2_amd", "csrc")
    src = [os.path.join(csrc, "waveglow_fwd.hip"), os.path.join(csrc, "waveglow.hip"), os.path.join(EMU, "emu_runtime.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g0", "-w", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           "-I", EMU, "-x", "c++"] + src + ["-o", out])
    emu = ctypes.CDLL(out)
    assert emu.t2amd_emulated() == 1
    for name, at in native._argtypes().items():
        if hasattr(emu, name):
            fn = getattr(emu, name)
            fn.argtypes, fn.restype = at, ctypes.c_int
    emu.t2amd_last_error.restype = ctypes.c_char_p
    assert hasattr(emu, "t2amd_wg_head_f32") and hasattr(emu, "t2amd_wg_nll_f32")
    return emu


def _f32(rs, *shape, scale=1.0):
    return torch.from_numpy((scale * rs.randn(*shape)).astype(np.float32))


def test_emulated_head_ragged_early_boundary_matches_float64(forward_emu):
    rs = np.random.RandomState(0)
    wg = wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=3))
    G, C, B = 8, 64, 3
    rows, frames = [40, 64, 3], [2, 2, 1]                       # two utterances end inside a frame
    R = max(rows)
    rowb, rowr, offs, P = wg.forward_plan(rows, frames)
    valid = (rowb >= 0).numpy()
    skip = _f32(rs, P, C)
    end_w, end_b = _f32(rs, 8, C, scale=0.05), _f32(rs, 8, scale=0.05)
    mix_w = _f32(rs, 6, 6)
    start_w, start_b = _f32(rs, C, 3), _f32(rs, C)
    audio0 = _f32(rs, P, G)
    sentinel = 7.0
    audio = audio0.clone()
    h = torch.zeros(P, C)
    z = torch.full((B, G, R), sentinel)
    big = torch.full((B, 9, R), sentinel)
    log_s = big[:, 2:6]                                          # a channel slice of a larger buffer, as forward() passes
    with base._emulated(forward_emu):
        # closes a flow of 8 channels, emits an early output of 2 into z[:, 2:4], opens a flow of 6
        native.wg_head(rowb, rowr, audio, G, B, R, skip=skip, end_w=end_w, end_b=end_b, log_s=log_s, z=z, z_off=2, n_emit=2,
                       mix_w=mix_w, start_w=start_w, start_b=start_b, h=h)
    sk, a0 = skip.numpy().astype(np.float64), audio0.numpy().astype(np.float64)
    e = sk @ end_w.numpy().astype(np.float64).T + end_b.numpy()
    x = a0.copy()
    x[:, 4:] = np.exp(e[:, 4:]) * x[:, 4:] + e[:, :4]
    y = x[:, 2:] @ mix_w.numpy().astype(np.float64).T
    hh = y[:, :3] @ start_w.numpy().astype(np.float64).T + start_b.numpy()
    got_a, got_h = audio.numpy(), h.numpy()
    tol = 1e-5
    assert np.abs(got_a[valid, :6] - y[valid]).max() < tol * max(1.0, np.abs(y).max())
    assert np.array_equal(got_a[valid, 6:], a0[valid, 6:].astype(np.float32))
    assert np.array_equal(got_a[~valid], audio0.numpy()[~valid]), "halo rows of audio must be untouched"
    assert np.abs(got_h[valid] - hh[valid]).max() < tol * max(1.0, np.abs(hh).max())
    assert not got_h[~valid].any(), "halo rows (and the tail of a partial frame) of h must stay zero"
    zn, ln = z.numpy(), big.numpy()
    for b, Rb in enumerate(rows):
        pr = np.arange(offs[b], offs[b] + Rb)
        assert np.abs(zn[b, 2:4, :Rb] - x[pr, :2].T).max() < tol * max(1.0, np.abs(x).max())
        assert np.abs(ln[b, 2:6, :Rb] - e[pr, 4:].T).max() < tol
        assert (zn[b, 2:4, Rb:] == sentinel).all() and (ln[b, 2:6, Rb:] == sentinel).all()
    assert (zn[:, :2] == sentinel).all() and (zn[:, 4:] == sentinel).all()
    assert (ln[:, :2] == sentinel).all() and (ln[:, 6:] == sentinel).all()

    # the first call: the waveform by stride into grouped rows, W_0 and start_0
    wave = _f32(rs, B, G * R + 5)
    mix8, start8 = _f32(rs, 8, 8), _f32(rs, C, 4)
    audio, h = torch.full((P, G), sentinel), torch.zeros(P, C)
    with base._emulated(forward_emu):
        native.wg_head(rowb, rowr, audio, G, B, R, wave=wave, mix_w=mix8, start_w=start8, start_b=start_b, h=h)
    for b, Rb in enumerate(rows):
        pr = np.arange(offs[b], offs[b] + Rb)
        xa = wave.numpy()[b, :G * Rb].reshape(Rb, G).astype(np.float64)
        ya = xa @ mix8.numpy().astype(np.float64).T
        assert np.abs(audio.numpy()[pr] - ya).max() < tol * max(1.0, np.abs(ya).max())
        ha = ya[:, :4] @ start8.numpy().astype(np.float64).T + start_b.numpy()
        assert np.abs(h.numpy()[pr] - ha).max() < tol * max(1.0, np.abs(ha).max())
    assert (audio.numpy()[~valid] == sentinel).all() and not h.numpy()[~valid].any()

    # the last call: nothing to open, every remaining channel into the tail slice of z
    end4_w, end4_b = _f32(rs, 4, C, scale=0.05), _f32(rs, 4, scale=0.05)
    audio = audio0.clone()
    z = torch.full((B, G, R), sentinel)
    ls2 = torch.full((B, 2, R), sentinel)
    with base._emulated(forward_emu):
        native.wg_head(rowb, rowr, audio, G, B, R, skip=skip, end_w=end4_w, end_b=end4_b, log_s=ls2, z=z, z_off=4, n_emit=4)
    e4 = sk @ end4_w.numpy().astype(np.float64).T + end4_b.numpy()
    x4 = a0[:, :4].copy()
    x4[:, 2:] = np.exp(e4[:, 2:]) * x4[:, 2:] + e4[:, :2]
    assert torch.equal(audio, audio0)
    for b, Rb in enumerate(rows):
        pr = np.arange(offs[b], offs[b] + Rb)
        assert np.abs(z.numpy()[b, 4:, :Rb] - x4[pr].T).max() < tol * max(1.0, np.abs(x4).max())
        assert (z.numpy()[b, 4:, Rb:] == sentinel).all() and (z.numpy()[b, :4] == sentinel).all()


def test_emulated_nll_reduction_matches_float64_and_ignores_the_batch(forward_emu):
    rs = np.random.RandomState(1)
    B, R = 3, 5000                                               # three chunks of 2048 rows
    rows = [5000, 2049, 7]
    z, ls = _f32(rs, B, 8, R), _f32(rs, B, 11, R + 3, scale=0.1)[:, 1:10, :R]
    rows_t = torch.tensor(rows, dtype=torch.int32)
    with base._emulated(forward_emu):
        out = wgm._nll_sums(z, ls, rows_t).clone()
        none = wgm._nll_sums(z, None, rows_t).clone()
        alone = [wgm._nll_sums(z[b:b + 1, :, :n].contiguous(), ls[b:b + 1, :, :n].contiguous(),
                               torch.tensor([n], dtype=torch.int32)).clone() for b, n in enumerate(rows)]
    for b, n in enumerate(rows):
        zz = (z[b, :, :n].double() ** 2).sum().item()
        sl = ls[b, :, :n].double().sum().item()
        assert abs(out[b, 0].item() - zz) < 1e-12 * zz
        assert abs(out[b, 1].item() - sl) < 1e-12 * ls[b, :, :n].double().abs().sum().item()
        assert torch.equal(out[b], alone[b][0]), "an utterance's sums must not depend on its batch"
        assert none[b, 0] == out[b, 0] and none[b, 1] == 0.0


@pytest.mark.parametrize("ragged", [False, True])
def test_emulated_forward_nll_and_loss_match_restatement(forward_emu, ragged):
    ref = base._small_ref(seed=5)
    wg = wgm.WaveGlow.from_module(ref)
    g = torch.Generator().manual_seed(6)
    B, N = 2, 3
    mel = torch.randn(B, 80, N, generator=g)
    T = 256 * N if not ragged else 256 * N - 40
    audio = 0.3 * torch.randn(B, T, generator=g)
    lens = [T, 264] if ragged else None                          # 264 samples: one frame and a partial one
    with base._emulated(forward_emu):
        z, ls, ld = wg((mel, audio), lengths=lens)
        nll = wg.nll(mel, audio, sigma=0.8, lengths=lens)
        loss = wgm.WaveGlowLoss(0.8)((z, ls, ld))
        loss_cat = wgm.WaveGlowLoss(0.8)((z, [t.clone() for t in ls], [float(t) for t in ld]))
    assert z.shape == (B, 8, T // 8) and z.dtype == torch.float32
    with torch.no_grad():
        want = fr.forward_ragged(ref, mel.double(), audio.double(), lens or [T] * B)
    ls_max = max(t.abs().max().item() for t in want[1])
    print("max |log_s| %.3g" % ls_max)
    assert ls_max > 1e-2
    assert _rel(z, want[0]) < 1e-5
    for k in range(len(ls)):
        assert ls[k].shape == want[1][k].shape
        assert (ls[k].double() - want[1][k]).abs().max().item() < 1e-5
        assert abs(ld[k].item() - want[2][k].item()) < 1e-5 * max(1.0, abs(want[2][k].item()))
    if ragged:
        assert not z[1, :, 33:].any() and not any(t[1, :, 33:].any() for t in ls)
    want_loss = fr.loss(want, 0.8).item() if not ragged else None
    for b, t in enumerate(lens or [T] * B):
        with torch.no_grad():
            one = fr.loss(fr.forward(ref, mel[b:b + 1].double(), audio[b:b + 1, :t].double()), 0.8).item()
        print("utterance %d: nll %.7f, restatement %.7f" % (b, nll[b].item(), one))
        assert abs(nll[b].item() - one) < 1e-5 * abs(one)
    if not ragged:
        assert abs(loss.item() - want_loss) < 1e-5 * abs(want_loss)
        assert loss_cat.item() == loss.item()
    # the round trip through the emulated flow tails
    if not ragged:
        with base._emulated(forward_emu):
            back = wg.infer(mel, 1.0, z=wg.latents_to_noise(z))
        rel = _rel(back, audio)
        print("round trip: relative L2 %.3g" % rel)
        assert rel < 1e-5


def test_negative_determinant_gives_nan_log_det(native_lib):
    wg = wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=3))
    with torch.no_grad():
        wg.convinv[1].conv.weight[:, 0] *= -1.0
    with base._validate_only():
        ld = wg((torch.zeros(1, 80, 1), torch.zeros(1, 256)))[2]
    assert torch.isnan(ld[1]) and abs(ld[0].item()) < 1e-3 and abs(ld[2].item()) < 1e-3
