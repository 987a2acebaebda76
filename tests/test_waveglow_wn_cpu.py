"""WaveGlow under weight norm without a GPU: csrc/waveglow_wn.hip (the one-launch fold and its backward over a segment
table) run on the host stand-in of tests/hip_emu against float64 ``torch._weight_norm`` and its autograd; the g / v form of
``WaveGlow`` (keys, loading in both directions, apply / remove) against ``waveglow_ref.make_ref(weight_norm=True)``; the
whole ``training_loss(...).backward()`` of a weight-normed module (products stood in by float64 torch) against float64
autograd through that restatement; ``Mel2Samp``, the driver's configuration and the refusals."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import golden_util as gu
import test_waveglow_cpu as base
import test_waveglow_train_cpu as tr
import waveglow_ref as wr
from tacotron2_amd import native
from tacotron2_amd import waveglow as wgm

EMU = base.EMU
TOL = tr.TOL               # float64 products leave the f32 element work: the limit test_waveglow_train_cpu.py uses for it
# every row length that occurs (start: n_half = 1 .. 4; 64-channel and 256-channel res_skip / in_layers; cond_layer 640;
# in_layers 768), one that is no multiple of 4 above 64, and one longer than the rows a wave keeps in registers
LENGTHS = (1, 2, 3, 4, 64, 192, 256, 640, 768, 70, 1024)


@pytest.fixture(scope="module")
def wn_emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("waveglow_wn_emu") / "libwaveglow_wn_emu.so")
    csrc = os.path.join(gu.ROOT, "tacotron2_amd", "csrc")
    src = [os.path.join(csrc, n) for n in ("waveglow_wn.hip", "waveglow_bwd.hip", "waveglow_fwd.hip", "waveglow.hip")]
    src.append(os.path.join(EMU, "emu_runtime.cpp"))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g0", "-w", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           "-I", EMU, "-x", "c++"] + src + ["-o", out])
    emu = ctypes.CDLL(out)
    assert emu.t2amd_emulated() == 1
    for name, at in native._argtypes().items():
        if hasattr(emu, name):
            fn = getattr(emu, name)
            fn.argtypes, fn.restype = at, ctypes.c_int
    emu.t2amd_last_error.restype = ctypes.c_char_p
    for name in ("t2amd_wg_weight_norm_f32", "t2amd_wg_weight_norm_bwd_f32", "t2amd_wg_weight_norm_short"):
        assert hasattr(emu, name), name
    return emu


def _segments(rs, lengths=LENGTHS):
    """One (v, g, dw) per row length: 70 rows for the short ones (more than one work unit of 64), a few otherwise."""
    segs = []
    for ln in lengths:
        rows = 70 if ln <= 4 else 3
        segs.append((torch.from_numpy(rs.randn(rows, ln).astype(np.float32)),
                     torch.from_numpy((0.5 + rs.rand(rows, 1)).astype(np.float32)),
                     torch.from_numpy(rs.randn(rows, ln).astype(np.float32))))
    return segs


def _layout(segs, dw_shift=8):
    """Flat v / g / dw buffers and the table lines: tensors at multiples of 4 floats, dw in another layout."""
    lines, off, goff, dwoff = [], 0, 0, dw_shift
    for v, g, _ in segs:
        rows, ln = v.shape
        lines.append((off, goff, dwoff, rows, ln))
        off = -(-(off + rows * ln) // 4) * 4
        dwoff = -(-(dwoff + rows * ln) // 4) * 4 + 4
        goff += rows
    vb, gb, dwb = torch.zeros(off), torch.zeros(-(-goff // 4) * 4), torch.zeros(dwoff)
    for (o, go, do, rows, ln), (v, g, dw) in zip(lines, segs):
        vb[o:o + rows * ln] = v.reshape(-1)
        gb[go:go + rows] = g.reshape(-1)
        dwb[do:do + rows * ln] = dw.reshape(-1)
    return lines, vb, gb, dwb


def _fold(emu, lines, vb, gb):
    host, n_units = native.wg_weight_norm_table(lines)
    w, norm = torch.full_like(vb, 7.0), torch.full_like(gb, 7.0)
    with base._emulated(emu):
        native.wg_weight_norm(host.clone(), host, n_units, vb, gb, w, norm)
    return w, norm


def _bwd(emu, lines, dwb, vb, gb, norm, scale):
    host, n_units = native.wg_weight_norm_table(lines)
    dg, dv = torch.full_like(gb, 7.0), torch.full_like(vb, 7.0)
    with base._emulated(emu):
        native.wg_weight_norm_bwd(host.clone(), host, n_units, dwb, vb, gb, norm, dg, dv, scale)
    return dg, dv


def test_emulated_fold_matches_float64_weight_norm_alone_and_in_company(wn_emu):
    segs = _segments(np.random.RandomState(0))
    lines, vb, gb, _ = _layout(segs)
    w, norm = _fold(wn_emu, lines, vb, gb)
    assert native.wg_weight_norm_table(lines)[1] == sum(2 if s[0].shape[1] <= 4 else 3 for s in segs)
    for (o, go, _, rows, ln), (v, g, _) in zip(lines, segs):
        got, got_n = w[o:o + rows * ln].view(rows, ln), norm[go:go + rows]
        want = torch._weight_norm(v.double(), g.double(), 0)
        theirs = (torch._weight_norm(v, g, 0).double() - want).abs().max().item()
        ours = (got.double() - want).abs().max().item()
        n_theirs = (torch.norm_except_dim(v, 2, 0).double() - v.double().norm(dim=1, keepdim=True)).abs().max().item()
        n_ours = (got_n.double() - v.double().norm(dim=1)).abs().max().item()
        print("len %4d: fold error %.3g (torch float32 %.3g), norm error %.3g (torch %.3g)" % (ln, ours, theirs, n_ours, n_theirs))
        assert ours <= 4 * theirs, (ln, ours, theirs)
        assert n_ours <= 4 * max(n_theirs, float(np.spacing(np.float32(got_n.max().item())))), (ln, n_ours, n_theirs)
        # the same tensor alone in a table: identical bits
        l1, v1, g1, _ = _layout([(v, g, v)])
        w1, n1 = _fold(wn_emu, l1, v1, g1)
        assert torch.equal(w1[:rows * ln].view(rows, ln), got) and torch.equal(n1[:rows], got_n), ln
    # nothing outside the tensors is written, and a second run gives the same bits
    mask = torch.ones_like(w, dtype=torch.bool)
    for o, _, _, rows, ln in lines:
        mask[o:o + rows * ln] = False
    assert (w[mask] == 7.0).all() and (norm[sum(l[3] for l in lines):] == 7.0).all()
    w2, norm2 = _fold(wn_emu, lines, vb, gb)
    assert torch.equal(w, w2) and torch.equal(norm, norm2)


def test_emulated_fold_backward_matches_float64_autograd(wn_emu):
    segs = _segments(np.random.RandomState(1))
    lines, vb, gb, dwb = _layout(segs)
    _, norm = _fold(wn_emu, lines, vb, gb)
    scale = 0.5                                              # a power of two: scaling is exact, the errors compare as they are
    dg, dv = _bwd(wn_emu, lines, dwb, vb, gb, norm, scale)
    for (o, go, do, rows, ln), (v, g, dw) in zip(lines, segs):
        def grads(dtype):
            vv, gg = v.to(dtype).requires_grad_(True), g.to(dtype).requires_grad_(True)
            (torch._weight_norm(vv, gg, 0) * dw.to(dtype)).sum().mul(scale).backward()
            return gg.grad.double(), vv.grad.double()
        want_g, want_v = grads(torch.float64)
        their_g, their_v = grads(torch.float32)
        got_g, got_v = dg[go:go + rows].view(rows, 1), dv[o:o + rows * ln].view(rows, ln)
        eg, ev = (got_g.double() - want_g).abs().max().item(), (got_v.double() - want_v).abs().max().item()
        tg, tv = (their_g - want_g).abs().max().item(), (their_v - want_v).abs().max().item()
        print("len %4d: dg error %.3g (torch float32 %.3g), dv error %.3g (torch %.3g)" % (ln, eg, tg, ev, tv))
        floor_g = float(np.spacing(np.float32(want_g.abs().max().item())))     # torch's own error can be exactly zero on 3 rows
        assert eg <= 4 * max(tg, floor_g), (ln, eg, tg)
        assert ev <= 4 * tv, (ln, ev, tv)
        l1, v1, g1, d1 = _layout([(v, g, dw)], dw_shift=0)
        _, n1 = _fold(wn_emu, l1, v1, g1)
        dg1, dv1 = _bwd(wn_emu, l1, d1, v1, g1, n1, scale)
        assert torch.equal(dg1[:rows].view(rows, 1), got_g) and torch.equal(dv1[:rows * ln].view(rows, ln), got_v), ln
    dg0, dv0 = _bwd(wn_emu, lines, torch.zeros_like(dwb), vb, gb, norm, 1.0)
    for o, go, _, rows, ln in lines:
        assert (dg0[go:go + rows] == 0).all() and (dv0[o:o + rows * ln] == 0).all(), "a zero dw gives exact zeros"


def _small(weight_norm, seed=5):
    return wr.make_ref(seed=seed, weight_norm=weight_norm, **base.SMALL)


def test_keys_shapes_and_loading_both_ways_match_the_weight_normed_restatement():
    ref = wr.make_ref(C=64, L=4, seed=2, weight_norm=True)
    want = ref.state_dict()
    assert len(want) == 398 and sum(k.endswith('weight_g') for k in want) == 120
    wg = wgm.WaveGlow(80, 12, 8, 4, 2, dict(n_layers=4, n_channels=64, kernel_size=3), weight_norm=True)
    assert wg.weight_norm
    got = wg.state_dict()
    assert set(got) == set(want) and all(got[k].shape == want[k].shape for k in want)
    assert {n for n, _ in wg.named_parameters()} == {n for n, _ in ref.named_parameters()}
    assert all(isinstance(p, torch.nn.Parameter) and p.is_contiguous() for p in wg.parameters())
    wg.load_state_dict(want, strict=True)
    for k in want:
        assert torch.equal(wg.state_dict()[k], want[k]), k
    ref2 = wr.make_ref(C=64, L=4, seed=3, weight_norm=True)
    ref2.load_state_dict(wg.state_dict(), strict=True)
    # the switches: in place, both spellings, and the default stays the folded module
    folded = wgm.WaveGlow.from_module(ref)
    assert not folded.weight_norm and set(folded.state_dict()) == set(wr.folded_state_dict(ref))
    back = wgm.WaveGlow.remove_weightnorm(wg)
    assert back is wg and not wg.weight_norm
    for k, v in folded.state_dict().items():
        assert torch.equal(wg.state_dict()[k], v), k          # remove folds as torch.nn.utils.remove_weight_norm does
    wg.apply_weight_norm()
    for name, m in wg._wn_modules():
        w = folded.state_dict()[name + '.weight']
        assert torch.equal(m.weight_v, w) and torch.equal(m.weight_g, torch.norm_except_dim(w, 2, 0)), name
        assert m.weight_g.shape == (w.shape[0], 1, 1)
    # apply then remove: the folded weights again, to within one fold (float32 rounding of v g / ||v|| with g = ||v||)
    wg.remove_weight_norm()
    for k, v in folded.state_dict().items():
        err = (wg.state_dict()[k] - v).abs().max().item()
        assert err <= 4 * float(np.spacing(np.float32(v.abs().max().item()))), (k, err)
    # loading: fold by default, keep g / v on request, refuse a folded state dict in a weight-normed module
    kept = wgm.load_waveglow({'model': want}, weight_norm=True)
    assert kept.weight_norm and all(torch.equal(kept.state_dict()[k], want[k]) for k in want)
    assert not wgm.load_waveglow({'model': want}).weight_norm
    up = wgm.WaveGlow.from_state_dict(folded.state_dict(), weight_norm=True)
    assert up.weight_norm and torch.equal(up.WN[0].start.weight_v, folded.WN[0].start.weight)
    with pytest.raises(ValueError, match="apply_weight_norm"):
        kept.load_state_dict(folded.state_dict())
    folded.load_state_dict(want)                              # the reverse loads by folding, as before
    assert torch.equal(folded.WN[3].cond_layer.weight, wgm.fold_weight_norm(want)['WN.3.cond_layer.weight'])


def _wn_oracle(ref, mel, audio, lens, sigma):
    want_loss, grads = tr._oracle(ref, mel, audio, lens, sigma)
    assert any(n.endswith('weight_g') for n in grads)
    return want_loss, grads


@pytest.mark.parametrize("ragged", [False, True])
def test_emulated_weight_normed_training_loss_backward_matches_float64_autograd(wn_emu, ragged):
    ref = _small(True).double()
    wg = wgm.WaveGlow.from_module(ref, weight_norm=True)
    g = torch.Generator().manual_seed(6)
    B, N = 2, 3
    mel = torch.randn(B, 80, N, generator=g)
    T = 256 * N if not ragged else 256 * N - 40
    audio = 0.3 * torch.randn(B, T, generator=g)
    lens = [T, 264] if ragged else None
    sigma = 0.8
    want_loss, want = _wn_oracle(ref, mel, audio, lens, sigma)
    with tr._emulated_train(wn_emu):
        loss = wg.training_loss(mel, audio, sigma=sigma, lengths=lens)
        assert loss.requires_grad and loss.dtype == torch.float32 and loss.shape == ()
        loss.backward()
        folded = wgm.WaveGlow.from_state_dict(wgm.fold_weight_norm(wg.state_dict()))
        same = folded.training_loss(mel, audio, sigma=sigma, lengths=lens)
    print("loss %.7f, folded module %.7f, oracle %.7f" % (loss.item(), same.item(), want_loss))
    assert abs(loss.item() - same.item()) < TOL * abs(want_loss)
    assert abs(loss.item() - want_loss) < TOL * abs(want_loss)
    assert {n for n, _ in wg.named_parameters()} == set(want)
    worst = 0.0
    for n, p in wg.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
        r = tr._rel(p.grad, want[n])
        worst = max(worst, r)
        assert r < TOL, "%s: relative L2 %.3g" % (n, r)
    print("worst per-tensor relative L2 %.3g over %d tensors" % (worst, len(want)))


def test_weight_normed_training_loss_autograd_contract(wn_emu):
    wg = wgm.WaveGlow.from_module(_small(True).double(), weight_norm=True)
    g = torch.Generator().manual_seed(7)
    mel, audio = torch.randn(2, 80, 2, generator=g), 0.3 * torch.randn(2, 512, generator=g)
    frozen = wg.WN[1].cond_layer.weight_g
    frozen.requires_grad_(False)
    with tr._emulated_train(wn_emu):
        wg.training_loss(mel, audio).backward()
        g1 = {n: p.grad.clone() for n, p in wg.named_parameters() if p.grad is not None}
        (wg.training_loss(mel, audio) * 0.5).backward()           # adds half of it
        with torch.no_grad():
            nograd = wg.training_loss(mel, audio)
    assert frozen.grad is None and len(g1) == len(list(wg.parameters())) - 1
    assert wg.WN[1].cond_layer.weight_v.grad is not None
    for n, p in wg.named_parameters():
        if p is not frozen:
            assert tr._rel(p.grad, 1.5 * g1[n]) < 1e-6, n
    assert not nograd.requires_grad


def test_pack_cache_sees_g_and_v_moving(wn_emu):
    """An in-place step on g / v (version counters) and a raw-pointer step (the engine's weight generation, what
    FusedAdam bumps) both make the next pack fold again; the folded weights follow."""
    from tacotron2_amd import engine
    wg = wgm.WaveGlow.from_module(_small(True).double(), weight_norm=True)
    dev = torch.device('cpu')
    with base._emulated(wn_emu):
        pk = wg._packed(dev)
        assert wg._packed(dev) is pk
        w0 = wg.WN[0].cond_layer.weight.clone()
        want = torch._weight_norm(wg.WN[0].cond_layer.weight_v.detach(), wg.WN[0].cond_layer.weight_g.detach(), 0)
        assert (w0 - want).abs().max() < 1e-6
        with torch.no_grad():
            wg.WN[0].cond_layer.weight_g.mul_(2.0)
        assert wg._packed(dev) is not pk
        assert torch.equal(wg.WN[0].cond_layer.weight, 2.0 * w0)
        pk = wg._packed(dev)
        wg.WN[0].cond_layer.weight_g.data.view(-1).numpy()[:] *= 0.5          # behind torch's back, as a kernel writes
        assert wg._packed(dev) is pk
        engine.bump_weight_generation()
        assert wg._packed(dev) is not pk
        assert torch.equal(wg.WN[0].cond_layer.weight, w0)


def test_weight_norm_entry_points_refuse_bad_arguments(native_lib):
    err = base._err
    lines = [(0, 0, 0, 70, 3), (212, 70, 212, 3, 256)]
    host, n_units = native.wg_weight_norm_table(lines)
    assert n_units == 2 + 3 and host.tolist()[1][5] == 2
    v, g = torch.zeros(212 + 768), torch.zeros(76)
    w, norm, dg, dv, dw = torch.zeros_like(v), torch.zeros_like(g), torch.zeros_like(g), torch.zeros_like(v), torch.zeros_like(v)
    with pytest.raises(native.NativeError, match="no CPU path"):
        native.wg_weight_norm(host.clone(), host, n_units, v, g, w, norm)
    with base._validate_only():
        native.wg_weight_norm(host.clone(), host, n_units, v, g, w, norm)
        native.wg_weight_norm_bwd(host.clone(), host, n_units, dw, v, g, norm, dg, dv, 2.0)
        err(native.wg_weight_norm, host.clone(), host, n_units, v[:900], g, w, norm, match="reaches float 980")
        err(native.wg_weight_norm, host.clone(), host, n_units, v, g[:72], w, norm, match="reaches row 73")
        err(native.wg_weight_norm, host.clone(), host, n_units + 1, v, g, w, norm, match="work units")
        err(native.wg_weight_norm, host.clone().int(), host, n_units, v, g, w, norm, match="int64")
        err(native.wg_weight_norm, host.clone(), host, n_units, v.double(), g, w, norm, match="float32")
        bad = native.wg_weight_norm_table([(0, 0, 0, 70, 3), (210, 70, 212, 3, 256)])[0]
        err(native.wg_weight_norm, bad.clone(), bad, n_units, v, g, w, norm, match="multiple of 4")
        err(native.wg_weight_norm_bwd, host.clone(), host, n_units, dw[:500], v, g, norm, dg, dv, match="gradient buffer")
        lib = native.load()
        p = native.ptr
        t = host.clone()
        err(native._check, lib.t2amd_wg_weight_norm_f32(p(t, torch.int64), 2, n_units, None, p(g), p(w), p(norm), None), "x",
            match="null operand")
        err(native._check, lib.t2amd_wg_weight_norm_f32(p(t, torch.int64), 2, n_units, p(v[1:]), p(g), p(w), p(norm), None),
            "x", match="16-byte aligned")
        err(native._check, lib.t2amd_wg_weight_norm_f32(None, 2, n_units, p(v), p(g), p(w), p(norm), None), "x",
            match="null table")
        err(native._check, lib.t2amd_wg_weight_norm_bwd_f32(p(t, torch.int64), 0, n_units, p(dw), p(v), p(g), p(norm), p(dg),
                                                             p(dv), 1.0, None), "x", match="empty table")
        err(native._check, lib.t2amd_wg_weight_norm_bwd_f32(p(t, torch.int64), 2, n_units, p(dw), p(v), p(g), p(norm), None,
                                                             p(dv), 1.0, None), "x", match="null operand")
        # a weight-normed module end to end through the argument checks: g / v get gradients of their own shapes
        wg = wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=3), weight_norm=True)
        loss = wg.training_loss(torch.zeros(2, 80, 3), torch.zeros(2, 768))
        loss.backward()
        assert all(q.grad is not None and q.grad.shape == q.shape for q in wg.parameters())
        assert wg.infer(torch.zeros(1, 80, 2)).shape == (1, 512)


# ---------------------------------------------------------------------------------------------------------------
# Mel2Samp and the driver's configuration
# ---------------------------------------------------------------------------------------------------------------
def test_mel2samp_segments_padding_seed_and_synthetic_source(tmp_path):
    from scipy.io.wavfile import write
    from tacotron2_amd.mel2samp import Mel2Samp
    rs = np.random.RandomState(0)
    paths = []
    for i, n in enumerate((30000, 9000, 16000)):                   # longer, shorter and exactly one segment
        path = str(tmp_path / ("a%d.wav" % i))
        write(path, 22050, (8000 * rs.randn(n)).astype(np.int16))
        paths.append(path)
    lst = str(tmp_path / "files.txt")
    with open(lst, "w") as fh:
        fh.write("\n".join(paths) + "\n")
    ds = Mel2Samp(lst, segment_length=16000, seed=11)
    assert len(ds) == 3 and sorted(ds.audio_files) == sorted(paths)
    items = [ds[i] for i in range(3)]
    assert all(a.shape == (16000,) and a.dtype == torch.float32 and a.abs().max() <= 1.0 for a in items)
    short = items[ds.audio_files.index(paths[1])]
    assert (short[9000:] == 0).all() and short[:9000].abs().max() > 0, "a short recording is zero-padded at the end"
    again = Mel2Samp(lst, segment_length=16000, seed=11)
    assert again.audio_files == ds.audio_files
    assert all(torch.equal(again[i], items[i]) for i in range(3)), "same seed, same segments"
    other = Mel2Samp(lst, segment_length=16000, seed=12)
    long_i, long_j = ds.audio_files.index(paths[0]), other.audio_files.index(paths[0])
    assert not torch.equal(other[long_j], items[long_i])
    with pytest.raises(ValueError, match="sampling rate"):
        Mel2Samp(lst, sampling_rate=16000)[0]
    syn = Mel2Samp('synthetic:5', segment_length=4096, seed=3)
    assert len(syn) == 5 and all(22050 <= n <= 220500 for n in syn.synthetic_lengths)
    a0 = syn[0]
    assert a0.shape == (4096,) and a0.abs().max() > 0 and a0.abs().max() <= 1.0
    assert torch.equal(Mel2Samp('synthetic:5', segment_length=4096, seed=3)[0], a0)
    batch = syn.collate([syn[i] for i in range(4)])
    assert batch.shape == (4, 4096)
    assert syn.n_frames == 16 and Mel2Samp('synthetic:2').n_frames == 63


def test_driver_config_defaults_file_and_overrides(tmp_path):
    from tacotron2_amd import waveglow_train as wt
    cfg = wt.load_config(None, [])
    t, d, w = cfg['train_config'], cfg['data_config'], cfg['waveglow_config']
    assert (t['learning_rate'], t['sigma'], t['batch_size'], t['fp16_run']) == (1e-4, 1.0, 12, False)
    assert (d['segment_length'], d['sampling_rate'], d['mel_fmax']) == (16000, 22050, 8000.0)
    assert (w['n_flows'], w['n_group'], w['n_early_every'], w['n_early_size']) == (12, 8, 4, 2)
    assert w['WN_config'] == dict(n_layers=8, n_channels=256, kernel_size=3)
    assert cfg['dist_config'] == dict(dist_backend='nccl', dist_url='tcp://localhost:54321')
    path = str(tmp_path / "config.json")
    with open(path, "w") as fh:
        json.dump(dict(train_config=dict(batch_size=4, output_directory="out"), waveglow_config=dict(WN_config=dict(n_layers=4))), fh)
    cfg = wt.load_config(path, ["train_config.epochs=3", "learning_rate=2e-4", "waveglow_config.WN_config.n_channels=64",
                                "training_files=synthetic:24", "fp16_run=true", "precision=bf16x3"])
    assert cfg['train_config']['batch_size'] == 4 and cfg['train_config']['epochs'] == 3
    assert cfg['train_config']['learning_rate'] == 2e-4 and cfg['train_config']['fp16_run'] is True
    assert cfg['waveglow_config']['WN_config'] == dict(n_layers=4, n_channels=64, kernel_size=3)
    assert cfg['data_config']['training_files'] == 'synthetic:24'
    assert wt.precision_of(cfg['train_config']) == 'bf16x3'
    assert wt.precision_of(dict(fp16_run=True, precision=None)) == 'bf16' and wt.precision_of(dict(fp16_run=False)) == 'fp32'
    with pytest.raises(KeyError, match="no_such_key"):
        wt.load_config(None, ["no_such_key=1"])
    with pytest.raises(ValueError, match="key=value"):
        wt.load_config(None, ["batch_size"])
    with pytest.raises(ValueError, match="precision"):
        wt.precision_of(dict(fp16_run=False, precision='fp8'))
