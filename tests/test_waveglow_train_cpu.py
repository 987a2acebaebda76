"""WaveGlow's backward pass without a GPU: csrc/waveglow_bwd.hip run on the host stand-in of tests/hip_emu -- the flow head
backward and the gate backward directly against float64 autograd of the same arithmetic, and the whole
``WaveGlow.training_loss(...).backward()`` with the products stood in by float64 torch, full and ragged, against autograd
through the float64 restatement (tests/waveglow_fwd_ref.py); the refusals of the new entry points (validate-only) and the
autograd contract of ``training_loss`` (accumulation, upstream scalar, frozen parameters, no_grad)."""
import contextlib
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
# what is left with float64 products is the f32 element work: the limit the forward CPU tests use for the same situation
TOL = 1e-5


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.fixture(scope="module")
def train_emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("waveglow_bwd_emu") / "libwaveglow_bwd_emu.so")
    csrc = os.path.join(gu.ROOT, "tacotron2_amd", "csrc")
    src = [os.path.join(csrc, n) for n in ("waveglow_bwd.hip", "waveglow_fwd.hip", "waveglow.hip")]
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
    for name in ("t2amd_wg_head_bwd_f32", "t2amd_wg_partial_sum_f32", "t2amd_wg_gate_bwd_f32", "t2amd_wg_head_save_f32"):
        assert hasattr(emu, name), name
    return emu


@contextlib.contextmanager
def _emulated_train(emu):
    """base._emulated plus float64 stand-ins of the products the training path adds (the element kernels run emulated)."""
    names = ("gemm", "splitk_reduce2d", "colsum", "wg_gated", "wg_res_skip", "wg_dgrad")
    with base._emulated(emu):
        saved = tuple(getattr(native, n) for n in names)
        fwd_gemm, fwd_gated, fwd_res_skip = native.gemm, native.wg_gated, native.wg_res_skip

        def gemm(Cm, A, B, a_km=False, b_kn=False, accumulate=False, bias=None, convA=None, splitk=1, partials=None,
                 fast=0, **kw):
            if not (a_km or b_kn or accumulate or splitk > 1):
                return fwd_gemm(Cm, A, B, bias=bias, convA=convA, fast=fast, **kw)
            r = (A.double().t() if a_km else A.double()) @ (B.double() if b_kn else B.double().t())
            if splitk > 1:
                part = partials[:splitk * r.numel()].view(splitk, -1)
                part.zero_()
                part[splitk - 1].copy_(r.reshape(-1))
            else:
                Cm.copy_(Cm.double() + r if accumulate else r)

        def splitk_reduce2d(partials, nsplit, out, accumulate=False):
            r = partials[:nsplit * out.numel()].view(nsplit, -1).double().sum(0).view(out.shape)
            out.copy_(out.double() + r if accumulate else r)

        def colsum(x, ws, out, accumulate=False):
            r = x.double().sum(0)
            out.copy_(out.double() + r if accumulate else r)

        def wg_gated(X, W, bias, dil, cnd, acts, precision, gate=None):
            fwd_gated(X, W, bias, dil, cnd, acts, precision)
            if gate is not None:
                C = acts.shape[1]
                A = torch.cat([base._shifted(X, -dil), X, base._shifted(X, dil)], 1).double()
                pre = (A @ W.double().t() + bias.double()).view(-1, C // 32, 2, 32)
                gate[:, :C] = torch.tanh(pre[:, :, 0].reshape(-1, C) + cnd[:, :C].double()).float()
                gate[:, C:] = torch.sigmoid(pre[:, :, 1].reshape(-1, C) + cnd[:, C:].double()).float()

        def wg_res_skip(acts, W, bias, h, skip, skip_store, rowb, precision, h_out=None):
            if h_out is None:
                return fwd_res_skip(acts, W, bias, h, skip, skip_store, rowb, precision)
            before = h.clone()
            fwd_res_skip(acts, W, bias, h, skip, skip_store, rowb, precision)
            ok = rowb[:h.shape[0]] >= 0
            h_out[ok] = h[ok]
            h.copy_(before)

        def wg_dgrad(d_pre, Wt, dil, dh, store, rowb, precision):
            A = torch.cat([base._shifted(d_pre, -dil), d_pre, base._shifted(d_pre, dil)], 1).double()
            r = A @ Wt.double().t()
            ok = rowb[:dh.shape[0]] >= 0
            dh[ok] = (r[ok] if store else dh.double()[ok] + r[ok]).float()

        for n, f in zip(names, (gemm, splitk_reduce2d, colsum, wg_gated, wg_res_skip, wg_dgrad)):
            setattr(native, n, f)
        try:
            yield
        finally:
            for n, f in zip(names, saved):
                setattr(native, n, f)


def _f32(rs, *shape, scale=1.0):
    return torch.from_numpy((scale * rs.randn(*shape)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------
# the element kernels alone
# ---------------------------------------------------------------------------------------------------------------
def _head_case(emu, rs, plan, G, C, B, R, n_in, n_emit, first=False):
    """One head call forward (emulated, keeping its rows) and backward, against float64 autograd of the head's arithmetic
    with random upstream gradients.  n_in = 0: the first call (the waveform); n_emit == n_in: the last one."""
    rowb, rowr, offs, P, valid = plan
    n_cur = n_in if not first else G
    n_out = n_cur - n_emit
    vt = torch.from_numpy(valid)
    c1, c2 = 0.37, -0.11
    skip = _f32(rs, P, C)
    a_prev = _f32(rs, P, G)                                     # the a rows of the call before (the coupling's input)
    wave = _f32(rs, B, G * R)
    end_w, end_b = _f32(rs, max(n_in, 2), C, scale=0.05), _f32(rs, max(n_in, 2), scale=0.05)
    mix_w = _f32(rs, n_out, n_out) if n_out else None
    start_w, start_b = (_f32(rs, C, n_out // 2), _f32(rs, C)) if n_out else (None, None)
    dh0 = _f32(rs, P, C)
    dA_in = _f32(rs, P, G)
    sentinel = 7.0
    audio = a_prev.clone()
    h = torch.zeros(P, C)
    z = torch.zeros(B, G, R)
    log_s = torch.zeros(B, max(n_in // 2, 1), R)
    save = torch.full((P, 2 * G), sentinel)
    fwd = dict(z=z if n_emit else None, z_off=0, n_emit=n_emit)
    if n_out:
        fwd.update(mix_w=mix_w, start_w=start_w, start_b=start_b, h=h)
    if first:
        fwd.update(wave=wave)
    else:
        fwd.update(skip=skip, end_w=end_w, end_b=end_b, log_s=log_s)
    dA = dA_in.clone()
    d_skip = torch.full((P, 2 * C), sentinel)[:, C:]             # a column block of a wider buffer, as the module passes it
    npart = native.wg_head_bwd_sizes(C, 0 if first else n_in, n_out)
    with base._emulated(emu):
        native.wg_head(rowb, rowr, audio, G, B, R, save=save, **fwd)
        nblk = -(-P // native.wg_head_bwd_rows())
        partial = torch.full((nblk * npart,), sentinel)
        kw = {}
        if not first:
            kw.update(skip=skip, end_w=end_w, log_s=log_s, a_in=a_prev, dA=dA, d_skip=d_skip)
        if n_out:
            kw.update(dA=dA, dh0=dh0, mix_w=mix_w, start_w=start_w, a_sv=save[:, G:])
        nb, n = native.wg_head_bwd(rowb, rowr, G, B, R, c1, c2, save[:, :G], partial, n_emit=n_emit, **kw)
        small = torch.full((npart,), sentinel)
        native.wg_partial_sum(partial, nb, n, small)
    assert (nb, n) == (nblk, npart)
    assert (save[~vt] == sentinel).all(), "halo rows of the kept rows must be untouched"

    # float64 autograd of the same arithmetic
    leaves = {}

    def leaf(name, t):
        leaves[name] = t.double().clone().requires_grad_(True)
        return leaves[name]

    if first:
        x = torch.zeros(P, G, dtype=torch.float64)
        for b in range(B):
            nb_ = int((rowb == b).sum())
            x[offs[b]:offs[b] + nb_] = wave[b, :G * nb_].view(nb_, G).double()
        S = torch.zeros((), dtype=torch.float64)
    else:
        a = leaf('a_in', a_prev[:, :n_in])
        e = leaf('skip', skip) @ leaf('end_w', end_w[:n_in]).t() + leaf('end_b', end_b[:n_in])
        nh = n_in // 2
        x = torch.cat([a[:, :nh], torch.exp(e[:, nh:]) * a[:, nh:] + e[:, :nh]], 1)
        S = c2 * e[vt][:, nh:].sum()
    S = S + 0.5 * c1 * (x[vt][:, :n_emit] ** 2).sum()
    if n_out:
        y = x[:, n_emit:] @ leaf('mix_w', mix_w).t()
        hh = y[:, :n_out // 2] @ leaf('start_w', start_w).t() + leaf('start_b', start_b)
        S = S + (dA_in[:, :n_out].double() * y)[vt].sum() + (dh0.double() * hh)[vt].sum()
    S.backward()
    assert (save[vt][:, :n_cur].double() - x[vt].detach()).abs().max() < TOL * max(1.0, x.abs().max().item())

    def close(got, name, shape=None):
        want = leaves[name].grad
        got = got.reshape(want.shape) if shape is None else got
        err = (got.double() - want).abs().max().item()
        assert err < TOL * max(1.0, want.abs().max().item()), (name, err)

    o = 0
    if not first:
        close(small[o:o + n_in * C], 'end_w')
        close(small[o + n_in * C:o + n_in * C + n_in], 'end_b')
        o += n_in * C + n_in
        want = leaves['skip'].grad
        assert (d_skip[vt].double() - want[vt]).abs().max() < TOL * max(1.0, want.abs().max().item())
        assert (d_skip[~vt] == sentinel).all(), "halo rows of d_skip must be untouched"
        want = leaves['a_in'].grad
        assert (dA[vt][:, :n_in].double() - want[vt]).abs().max() < TOL * max(1.0, want.abs().max().item())
        assert torch.equal(dA[~vt], dA_in[~vt]) and torch.equal(dA[:, n_in:], dA_in[:, n_in:])
    else:
        assert torch.equal(dA, dA_in)
    if n_out:
        nh2 = n_out // 2
        close(small[o:o + C * nh2], 'start_w')
        close(small[o + C * nh2:o + C * nh2 + C], 'start_b')
        close(small[o + C * nh2 + C:], 'mix_w')
    assert not (small == sentinel).any()
    for t in leaves.values():
        assert t.grad.abs().max() > 0


def test_emulated_head_backward_ragged_early_boundary_matches_float64_autograd(train_emu):
    rs = np.random.RandomState(0)
    wg = wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=3))
    G, C, B = 8, 64, 3
    rows, frames = [40, 64, 3], [2, 2, 1]                       # two utterances end inside a frame
    rowb, rowr, offs, P = wg.forward_plan(rows, frames)
    plan = (rowb, rowr, offs, P, (rowb >= 0).numpy())
    _head_case(train_emu, rs, plan, G, C, B, max(rows), n_in=8, n_emit=2)             # an early boundary: 8 -> 6 channels
    _head_case(train_emu, rs, plan, G, C, B, max(rows), n_in=6, n_emit=0)             # a plain boundary
    _head_case(train_emu, rs, plan, G, C, B, max(rows), n_in=0, n_emit=0, first=True)  # the waveform: nothing to close
    _head_case(train_emu, rs, plan, G, C, B, max(rows), n_in=4, n_emit=4)             # the last call: nothing to open


def test_emulated_gate_backward_matches_float64(train_emu):
    rs = np.random.RandomState(1)
    M, C = 70, 64
    d_acts = _f32(rs, M, C)
    u, v = _f32(rs, M, C).double().requires_grad_(True), _f32(rs, M, C).double().requires_grad_(True)
    t, s = torch.tanh(u), torch.sigmoid(v)
    rowb = torch.from_numpy((rs.rand(M) > 0.2).astype(np.int32) - 1)
    ok = rowb >= 0
    ((t * s) * d_acts.double())[ok].sum().backward()
    gate = torch.cat([t.detach(), s.detach()], 1).float()
    slab = torch.full((M, 6 * C), 7.0)
    d_pre = slab[:, 2 * C:4 * C]                                  # a layer's slice of the cond slab
    acts = torch.full((M, C), 7.0)
    with base._emulated(train_emu):
        native.wg_gate_bwd(d_acts, gate, rowb, d_pre, acts)
    assert (d_pre[ok][:, :C].double() - u.grad[ok]).abs().max() < TOL
    assert (d_pre[ok][:, C:].double() - v.grad[ok]).abs().max() < TOL
    assert (acts[ok].double() - (t * s).detach()[ok]).abs().max() < TOL
    assert (d_pre[~ok] == 7.0).all() and (acts[~ok] == 7.0).all(), "rows that are not real must not be written"
    assert (slab[:, :2 * C] == 7.0).all() and (slab[:, 4 * C:] == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------
# the whole training_loss(...).backward()
# ---------------------------------------------------------------------------------------------------------------
def _oracle(ref, mel, audio, lens, sigma):
    """Autograd through the float64 restatement; ragged: the NLL numerators of the utterances over the real samples."""
    ref.zero_grad()
    if lens is None:
        out = fr.forward(ref, mel.double(), audio.double())
        ls_max = max(t.abs().max().item() for t in out[1])
        loss = fr.loss(out, sigma)
    else:
        z, ls, ld = fr.forward_ragged(ref, mel.double(), audio.double(), lens)
        ls_max = max(t.abs().max().item() for t in ls)
        loss = fr.loss((z, ls, ld), sigma) * z.numel() / (z.shape[1] * sum(t // z.shape[1] for t in lens))
    loss.backward()
    grads = {n: p.grad.clone() for n, p in ref.named_parameters()}
    assert ls_max > 1e-2, "the couplings must not be the identity"
    for n, g in grads.items():
        assert g is not None and g.abs().max() > 0, "the oracle's gradient of %s is zero" % n
    return loss.item(), grads


@pytest.mark.parametrize("ragged", [False, True])
def test_emulated_training_loss_backward_matches_float64_autograd(train_emu, ragged):
    ref = wr.make_ref(C=64, L=4, seed=5, weight_norm=False).double()
    wg = wgm.WaveGlow.from_module(ref)
    g = torch.Generator().manual_seed(6)
    B, N = 2, 3
    mel = torch.randn(B, 80, N, generator=g)
    T = 256 * N if not ragged else 256 * N - 40
    audio = 0.3 * torch.randn(B, T, generator=g)
    lens = [T, 264] if ragged else None                          # 264 samples: one frame and a partial one
    sigma = 0.8
    want_loss, want = _oracle(ref, mel, audio, lens, sigma)
    with _emulated_train(train_emu):
        loss = wg.training_loss(mel, audio, sigma=sigma, lengths=lens)
        assert loss.requires_grad and loss.dtype == torch.float32 and loss.shape == ()
        with torch.no_grad():
            plain = wg.training_loss(mel, audio, sigma=sigma, lengths=lens)
        if not ragged:
            same = wgm.WaveGlowLoss(sigma)(wg((mel, audio)))
            assert same.item() == loss.item(), "the saving forward runs forward's launches"
        loss.backward()
    assert not plain.requires_grad and plain.item() == loss.item()
    print("loss %.7f, oracle %.7f" % (loss.item(), want_loss))
    assert abs(loss.item() - want_loss) < TOL * abs(want_loss)
    names = [n for n, _ in wg.named_parameters()]
    assert set(names) == set(want)
    worst = 0.0
    for n, p in wg.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == torch.float32, n
        r = _rel(p.grad, want[n])
        worst = max(worst, r)
        assert r < TOL, "%s: relative L2 %.3g" % (n, r)
    print("worst per-tensor relative L2 %.3g over %d tensors" % (worst, len(names)))


def test_training_loss_autograd_contract(train_emu):
    ref = base._small_ref(seed=5, weight_norm=False)
    wg = wgm.WaveGlow.from_module(ref)
    g = torch.Generator().manual_seed(7)
    mel, audio = torch.randn(2, 80, 2, generator=g), 0.3 * torch.randn(2, 512, generator=g)
    frozen = wg.WN[1].cond_layer.weight
    frozen.requires_grad_(False)
    with _emulated_train(train_emu):
        wg.training_loss(mel, audio).backward()
        g1 = {n: p.grad.clone() for n, p in wg.named_parameters() if p.grad is not None}
        (wg.training_loss(mel, audio) * 0.5).backward()           # adds half of it
        for p in wg.parameters():
            p.requires_grad_(False)
        nograd = wg.training_loss(mel, audio)
    assert frozen.grad is None and len(g1) == len(list(wg.parameters())) - 1
    for n, p in wg.named_parameters():
        if p is not frozen:
            assert _rel(p.grad, 1.5 * g1[n]) < 1e-6, n
    assert not nograd.requires_grad


def test_training_loss_and_new_entry_points_refuse_bad_arguments(native_lib):
    wg = wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=3))
    mel = torch.zeros(2, 80, 3)
    with pytest.raises(native.NativeError, match="no CPU path"):
        wg.training_loss(mel, torch.zeros(2, 768))
    err = base._err
    with base._validate_only():
        loss = wg.training_loss(mel, torch.zeros(2, 768))
        assert loss.shape == () and loss.requires_grad
        loss.backward()
        assert all(p.grad is not None and p.grad.shape == p.shape for p in wg.parameters())
        with pytest.raises(ValueError, match="audio require grad"):
            wg.training_loss(mel, torch.zeros(2, 768, requires_grad=True))
        with pytest.raises(ValueError, match="mels require grad"):
            wg.training_loss(mel.clone().requires_grad_(True), torch.zeros(2, 768))
        with pytest.raises(ValueError, match="multiples of n_group"):
            wg.training_loss(mel, torch.zeros(2, 768), lengths=[768, 100])
        with pytest.raises(ValueError, match="do not fit"):
            wg.training_loss(mel, torch.zeros(2, 768), lengths=[768, 776])
        with pytest.raises(ValueError, match=r"at most 256 \* N = 768"):
            wg.training_loss(mel, torch.zeros(2, 776))
        assert wg.saved_state_bytes(100, 6) == 4 * (100 * (4 * (3 * 64 * 2 + 64) + 16 * 5) + 4 * 80 * 6)

        P, C, G, B, R = 80, 64, 8, 2, 30
        rowb = torch.zeros(P, dtype=torch.int32)
        X, acts, skip, h = (torch.zeros(P, C) for _ in range(4))
        cnd, gate = torch.zeros(P, 2 * C), torch.zeros(P, 2 * C)
        # the layer product's training outputs and the data-gradient mode
        native.wg_gated(X, torch.zeros(2 * C, 3 * C), torch.zeros(2 * C), 2, cnd, acts, 0, gate=gate)
        err(native.wg_gated, X, torch.zeros(2 * C, 3 * C), torch.zeros(2 * C), 2, cnd, acts, 0, gate=torch.zeros(P, C),
            match="gate")
        native.wg_res_skip(acts, torch.zeros(2 * C, C), torch.zeros(2 * C), h, skip, True, rowb, 1, h_out=torch.zeros(P, C))
        err(native.wg_res_skip, acts, torch.zeros(C, C), torch.zeros(C), None, skip, True, rowb, 1, h_out=h, match="h_out")
        err(native.wg_res_skip, acts, torch.zeros(2 * C, C), torch.zeros(2 * C), h, skip, True, rowb, 1,
            h_out=torch.zeros(P, 32), match="h_out")
        native.wg_dgrad(cnd, torch.zeros(C, 6 * C), 2, h, True, rowb, 2)
        err(native.wg_dgrad, cnd, torch.zeros(C, 3 * C), 2, h, True, rowb, 0, match="shape mismatch")
        err(native.wg_dgrad, cnd, torch.zeros(C, 6 * C), 2, h, True, rowb, 3, match="precision")
        err(native.wg_dgrad, cnd, torch.zeros(C, 6 * C), 2, h.double(), True, rowb, 0, match="float32")
        lib = native.load()
        p = native.ptr
        err(native._check, lib.t2amd_wg_layer_train_f32(p(cnd), 2 * C, p(gate), None, P, C, 2 * C, 3, 1, 2, None, 0, None, 0,
                                                         None, 0, 0, None, 0, 0, p(rowb, torch.int32), None, 0, None, 0, 0,
                                                         None), "x", match="data gradient needs h")
        err(native._check, lib.t2amd_wg_layer_train_f32(p(X), C, p(gate), p(gate), P, 2 * C, C, 1, 1, 1, None, 0, None, 0,
                                                         p(h), C, C, p(skip), C, 0, p(rowb, torch.int32), p(gate), 2 * C,
                                                         None, 0, 0, None), "x", match="gate values")
        # the head that keeps its rows
        audio = torch.zeros(P, G)
        z, ls = torch.zeros(B, G, R), torch.zeros(B, 4, R)
        end = dict(skip=skip, end_w=torch.zeros(8, C), end_b=torch.zeros(8), log_s=ls)
        nxt = dict(mix_w=torch.zeros(6, 6), start_w=torch.zeros(C, 3), start_b=torch.zeros(C), h=h)
        native.wg_head(rowb, rowb, audio, G, B, R, z=z, n_emit=2, save=torch.zeros(P, 2 * G), **end, **nxt)
        err(native.wg_head, rowb, rowb, audio, G, B, R, z=z, n_emit=2, save=torch.zeros(P, G), **end, **nxt, match="save")
        # the head backward
        sv = torch.zeros(P, 2 * G)
        dA, dh0, d_skip = torch.zeros(P, G), torch.zeros(P, C), torch.zeros(P, C)
        assert native.wg_head_bwd_rows() == 64
        n = native.wg_head_bwd_sizes(C, 8, 6)
        assert n == 8 * C + 8 + C * 3 + C + 36
        part = torch.zeros(2 * n)
        bend = dict(skip=skip, end_w=torch.zeros(8, C), log_s=ls, a_in=sv[:, G:], dA=dA, d_skip=d_skip)
        bnxt = dict(dh0=dh0, mix_w=torch.zeros(6, 6), start_w=torch.zeros(C, 3), a_sv=sv[:, G:])
        assert native.wg_head_bwd(rowb, rowb, G, B, R, 1.0, -1.0, sv[:, :G], part, n_emit=2, **bend, **bnxt) == (2, n)
        native.wg_head_bwd(rowb, rowb, G, B, R, 1.0, -1.0, sv[:, :G], part, n_emit=8, **bend)
        native.wg_head_bwd(rowb, rowb, G, B, R, 1.0, -1.0, sv[:, :G], part, dA=dA, dh0=dh0, mix_w=torch.zeros(8, 8),
                           start_w=torch.zeros(C, 4), a_sv=sv[:, G:])
        err(native.wg_head_bwd, rowb, rowb, G, B, R, 1.0, -1.0, sv[:, :G], part[:n], n_emit=2, **bend, **bnxt,
            match="partial holds")
        err(native.wg_head_bwd, rowb, rowb, G, B, R, 1.0, -1.0, sv[:, :G], part, n_emit=4, **bend, **bnxt, match="n_out = 4")
        err(native.wg_head_bwd, rowb, rowb, G, B, R, 1.0, -1.0, sv[:, :G], part, n_emit=3, **bend, match="n_emit")
        err(native.wg_head_bwd, rowb, rowb, G, B, R, 1.0, -1.0, sv[:, :G], part, n_emit=2, **bend,
            match="emitted every remaining channel")
        err(native.wg_head_bwd, rowb, rowb, G, B, R, 1.0, -1.0, sv[:, :G], part, match="neither a flow to close")
        err(native.wg_head_bwd, rowb, rowb, 7, B, R, 1.0, -1.0, sv[:, :G], part, n_emit=8, **bend, match="n_group")
        err(native.wg_head_bwd, rowb, rowb, G, B, R, 1.0, -1.0, sv[:40, :G], part, n_emit=8, **bend, match="x_sv has 40 rows")
        err(native.wg_head_bwd, rowb, rowb, G, B, R, 1.0, -1.0, sv[:, :G], part, n_emit=8,
            **dict(bend, log_s=torch.zeros(B, 3, R)), match="log_s")
        err(native.wg_head_bwd, rowb, rowb, G, B, R, 1.0, -1.0, sv[:, :G], torch.zeros(2 * 8 * 601), n_emit=8,
            **dict(bend, end_w=torch.zeros(8, 600), skip=torch.zeros(P, 600), d_skip=torch.zeros(P, 600)), match="C must")
        err(native.wg_head_bwd, rowb, rowb, G, B, R, 1.0, -1.0, sv[:, :G].double(), part, n_emit=8, **bend, match="float32")
        err(native._check, lib.t2amd_wg_head_bwd_f32(None, C, C, p(bend['end_w']), 8, p(ls), 4 * R, R, p(sv), 2 * G, p(sv),
                                                      2 * G, None, 0, p(dA), G, None, 0, None, None, 8, p(d_skip), C, p(part),
                                                      8 * C + 8, p(rowb, torch.int32), p(rowb, torch.int32), P, G, B, R, 1.0,
                                                      -1.0, None), "x", match="null operand")
        err(native._check, lib.t2amd_wg_head_bwd_f32(p(skip), C, C, p(bend['end_w']), 8, p(ls), 4 * R, R, p(sv), 2 * G, p(sv),
                                                      2 * G, None, 0, p(dA), G, None, 0, None, None, 8, p(d_skip), C, p(part),
                                                      8 * C, p(rowb, torch.int32), p(rowb, torch.int32), P, G, B, R, 1.0,
                                                      -1.0, None), "x", match="npart")
        # the partial sums and the gate backward
        native.wg_partial_sum(part, 2, n, torch.zeros(n))
        err(native.wg_partial_sum, part, 3, n, torch.zeros(n), match="partials")
        err(native.wg_partial_sum, part, 2, n, torch.zeros(n + 1), match="outputs")
        err(native.wg_partial_sum, part.double(), 2, n, torch.zeros(n), match="float32")
        native.wg_gate_bwd(acts, gate, rowb, cnd, X)
        err(native.wg_gate_bwd, acts, torch.zeros(P, C), rowb, cnd, X, match="shape mismatch")
        err(native.wg_gate_bwd, acts, gate, rowb[:10], cnd, X, match="shape mismatch")
        err(native.wg_gate_bwd, acts, gate, rowb.long(), cnd, X, match="int32")
        err(native._check, lib.t2amd_wg_gate_bwd_f32(p(acts), C, p(gate), C, p(rowb, torch.int32), P, C, p(cnd), 2 * C, p(X),
                                                      C, None), "x", match="rows too short")


def test_pack_cache_sees_raw_pointer_optimizer_steps():
    """FusedAdam updates the weights through raw pointers, which torch's version counters do not see: it bumps the engine's
    weight generation, and the packed weights must be rebuilt after it."""
    from tacotron2_amd import engine
    wg = wgm.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=3))
    dev = torch.device('cpu')
    pk = wg._packed(dev)
    assert wg._packed(dev) is pk
    engine.bump_weight_generation()
    assert wg._packed(dev) is not pk
    assert all(p.is_contiguous() for p in wg.parameters()), "FusedAdam takes contiguous parameters only"
