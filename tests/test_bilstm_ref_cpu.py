"""The yardstick of the encoder bi-LSTM kernel tests (tests/bilstm_ref.py) against the operation itself, and the argument
checks of the five native forms -- both without a GPU.

  * The float64 restatement equals float64 ``torch.nn.LSTM(bidirectional=True, batch_first=True)`` under
    ``pack_padded_sequence(enforce_sorted=False)`` to 1e-12 relative: outputs, DG (through an identity-projected input) and
    the W_hh / bias gradients that follow from DG.  This pins the reference the GPU tests use to nn.LSTM, not to this project's
    reading of it.
  * Under ``native.set_validate_only(True)`` the host checks of the launch chains, the one-utterance persistent forward and the
    batch-persistent forward / BPTT accept and refuse the geometries their contracts name (include/tacotron2_amd.h).
"""
import pytest
import torch

import bilstm_ref as br

REL = 1e-12


def _close(a, b, what):
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    assert err <= REL * max(scale, 1.0), (what, err, scale)


def _draw(B, T, H, seed):
    g = torch.Generator().manual_seed(seed)
    Whh = [torch.randn(4 * H, H, generator=g, dtype=torch.float64) * 0.2 for _ in range(2)]
    GX = [torch.randn(B, T, 4 * H, generator=g, dtype=torch.float64) * 0.7 for _ in range(2)]
    dout = torch.randn(B, T, 2 * H, generator=g, dtype=torch.float64) * 0.3
    return g, Whh, GX, dout


@pytest.mark.parametrize("name,B,T,H,lens", [
    ("ragged sorted", 6, 9, 8, "sorted"),
    ("ragged unsorted", 7, 9, 8, "unsorted"),
    ("edge: a length of 1, full lengths, equal neighbours", 7, 9, 8, "edge"),
    ("one utterance of length 1 among longer ones", 4, 6, 5, [6, 1, 4, 4]),
    ("all lengths equal to T", 5, 7, 8, [7] * 5),
    ("T = 1", 3, 1, 8, [1, 1, 1]),
    ("one utterance", 1, 5, 12, [5]),
])
def test_restatement_equals_nn_lstm_in_float64(name, B, T, H, lens):
    g, Whh, GX, dout = _draw(B, T, H, 100 * B + T)
    if isinstance(lens, str):
        lens = br.lengths(lens, B, T, g)
    assert max(lens) == T and len(lens) == B
    ref = br.bilstm(GX, Whh, lens, dout)
    out, DG, dW, db = br.torch_bilstm(GX, Whh, lens, dout)
    _close(ref.out, out, "out")
    valid = torch.arange(T).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)
    assert torch.all(ref.out[~valid] == 0)
    for d in range(2):
        _close(ref.DG[d], DG[d], "DG[%d]" % d)
        assert torch.all(ref.DG[d][~valid] == 0) and torch.all(ref.gates[d][~valid] == 0)
        assert torch.all(ref.C[d].transpose(0, 1)[~valid] == 0)
        rW, rb = br.weight_readings(ref.DG[d], ref.out[:, :, d * H:(d + 1) * H], lens, d)
        _close(rW, dW[d], "dW_hh[%d]" % d)
        _close(rb, db[d], "dbias[%d]" % d)
        # h = o * tanh(c): the saved gates and cell states are the ones the outputs were formed from
        o_gate = ref.gates[d][:, :, 3 * H:]
        _close(o_gate * torch.tanh(ref.C[d].transpose(0, 1)), ref.out[:, :, d * H:(d + 1) * H], "h from saved state")


def test_restatement_single_directions_are_the_halves_of_the_pair():
    """reverse = (0,) / (1,) alone (the q == NULL entries) are the two halves of the bidirectional run."""
    B, T, H = 5, 7, 8
    g, Whh, GX, dout = _draw(B, T, H, 5)
    lens = br.lengths("unsorted", B, T, g)
    both = br.bilstm(GX, Whh, lens, dout)
    for d in range(2):
        one = br.bilstm([GX[d]], [Whh[d]], lens, dout[:, :, d * H:(d + 1) * H], reverse=(d,))
        assert torch.equal(one.out, both.out[:, :, d * H:(d + 1) * H])
        assert torch.equal(one.DG[0], both.DG[d]) and torch.equal(one.C[0], both.C[d])


def test_float32_run_is_the_same_loop():
    """The yardstick run: same loop in float32, close to the float64 one and not identical to it."""
    B, T, H = 4, 9, 16
    g, Whh, GX, dout = _draw(B, T, H, 9)
    lens = br.lengths("sorted", B, T, g)
    r64, r32 = br.bilstm(GX, Whh, lens, dout), br.bilstm(GX, Whh, lens, dout, dtype=torch.float32)
    assert r32.out.dtype == torch.float32 and r32.DG[1].dtype == torch.float32
    e = float((r32.out.double() - r64.out).abs().max())
    assert 0 < e < 1e-5


# ------------------------------------------------------------------------------------------------------------------
# argument checks of the native forms (validate-only: host logic runs, no kernel is launched, tensors live on the CPU)
# ------------------------------------------------------------------------------------------------------------------
CUS = 256


def _descs(nv, B, T, H, dx_splits=4, T1=None, keep=None):
    """Forward + backward descriptors of both directions over CPU tensors (kept alive in ``keep``)."""
    out = []
    lens = torch.full((B,), T, dtype=torch.int32)
    for d in range(2):
        Td = T if (d == 0 or T1 is None) else T1
        z = lambda *s: torch.zeros(*s)
        t = dict(Whh=z(4 * H, H), WhhT=z(H, 4 * H), GX=z(B * Td, 4 * H), out=z(B * Td, H), C=z(Td, B, H), dout=z(B * Td, H),
                 DG=z(B * Td, 4 * H), dX=z(4, B, H), dc=z(B, H))
        keep.append((t, lens))
        desc = nv.LstmSeq()
        desc.B, desc.T, desc.H, desc.reverse = B, Td, H, d
        desc.Whh, desc.WhhT, desc.GX = nv.ptr(t["Whh"]), nv.ptr(t["WhhT"]), nv.ptr(t["GX"])
        desc.out, desc.ld_out = nv.ptr(t["out"]), H
        desc.C, desc.lens = nv.ptr(t["C"]), nv.ptr(lens, torch.int32)
        desc.dout, desc.ld_dout = nv.ptr(t["dout"]), H
        desc.DG, desc.dX, desc.dc, desc.dx_splits = nv.ptr(t["DG"]), nv.ptr(t["dX"]), nv.ptr(t["dc"]), dx_splits
        out.append(desc)
    return out


def _persistent_calls(nv, d, B, H):
    """The three persistent launches on descriptors d (both directions) -> list of (name, callable)."""
    mailbox = torch.zeros(4 * max(H, 64), dtype=torch.int64)
    flags = torch.zeros(max(nv.lstm_seq_batch_persistent_flag_words(B, max(H, 64), 2), 1), dtype=torch.int32)
    status = torch.zeros(1, dtype=torch.int32)
    return [("fwd2_persistent", lambda: nv.lstm_seq_fwd2_persistent(d[0], d[1], mailbox, status)),
            ("fwd2_batch_persistent", lambda: nv.lstm_seq_fwd2_batch_persistent(d[0], d[1], flags, status)),
            ("bwd2_batch_persistent", lambda: nv.lstm_seq_bwd2_batch_persistent(d[0], d[1], flags, status))]


def test_argument_checks_of_the_five_forms(native_lib):
    from tacotron2_amd import native as nv
    nv.set_validate_only(True)
    try:
        keep = []
        # a supported geometry passes everywhere (so that the refusals below are refusals of the geometry, not of the harness)
        d = _descs(nv, 1, 3, 128, keep=keep)
        nv.lstm_seq_fwd2(d[0], d[1])
        nv.lstm_seq_bwd2(d[0], d[1])
        nv.lstm_seq_fwd(d[1])
        nv.lstm_seq_bwd(d[1])
        assert nv.lstm_seq_persistent_supported(d[0]) is None
        assert nv.lstm_seq_batch_persistent_supported(d[0], 2, CUS) is None
        assert nv.lstm_seq_bwd2_batch_persistent_supported(d[0], 2, CUS) is None
        for name, call in _persistent_calls(nv, d, 1, 128):
            call()

        # H = 96: no multiple of 64 -- refused by both chains and by all three _supported calls
        d = _descs(nv, 1, 3, 96, keep=keep)
        with pytest.raises(nv.NativeError, match="multiple of 64"):
            nv.lstm_seq_fwd2(d[0], d[1])
        with pytest.raises(nv.NativeError, match="multiple of 64"):
            nv.lstm_seq_bwd2(d[0], d[1])
        for why in (nv.lstm_seq_persistent_supported(d[0]), nv.lstm_seq_batch_persistent_supported(d[0], 2, CUS),
                    nv.lstm_seq_bwd2_batch_persistent_supported(d[0], 2, CUS)):
            assert why is not None and "multiple of 64" in why, why

        # H = 320: the chains take any multiple of 64, the three persistent forms hold at most 256 units in registers
        d = _descs(nv, 1, 3, 320, keep=keep)
        nv.lstm_seq_fwd2(d[0], d[1])
        nv.lstm_seq_bwd2(d[0], d[1])
        for why in (nv.lstm_seq_persistent_supported(d[0]), nv.lstm_seq_batch_persistent_supported(d[0], 2, CUS),
                    nv.lstm_seq_bwd2_batch_persistent_supported(d[0], 2, CUS)):
            assert why is not None and "<= 256" in why, why
        for name, call in _persistent_calls(nv, d, 1, 320):
            with pytest.raises(nv.NativeError):
                call()

        # dx_splits: 0..4, and 2..4 must divide the 4H/64 k tiles -- 3 only at H = 192
        for H in (64, 128, 192, 256):
            d = _descs(nv, 2, 3, H, dx_splits=3, keep=keep)
            if H == 192:
                nv.lstm_seq_bwd2(d[0], d[1])
            else:
                with pytest.raises(nv.NativeError, match="dx_splits"):
                    nv.lstm_seq_bwd2(d[0], d[1])
            for ok in (0, 1, 2, 4):
                d = _descs(nv, 2, 3, H, dx_splits=ok, keep=keep)
                nv.lstm_seq_bwd2(d[0], d[1])
            d = _descs(nv, 2, 3, H, dx_splits=5, keep=keep)
            with pytest.raises(nv.NativeError, match="dx_splits"):
                nv.lstm_seq_bwd2(d[0], d[1])
            d[0].dx_splits = d[1].dx_splits = -1
            with pytest.raises(nv.NativeError, match="dx_splits"):
                nv.lstm_seq_bwd2(d[0], d[1])

        # two directions of different T
        d = _descs(nv, 1, 3, 64, T1=4, keep=keep)
        with pytest.raises(nv.NativeError, match="same length"):
            nv.lstm_seq_fwd2(d[0], d[1])
        with pytest.raises(nv.NativeError, match="same length"):
            nv.lstm_seq_bwd2(d[0], d[1])
        for name, call in _persistent_calls(nv, d, 1, 64):
            with pytest.raises(nv.NativeError, match="must match"):
                call()

        # B = 2: not the one-utterance form's
        d = _descs(nv, 2, 3, 64, keep=keep)
        why = nv.lstm_seq_persistent_supported(d[0])
        assert why is not None and "one utterance" in why
        calls = dict(_persistent_calls(nv, d, 2, 64))
        with pytest.raises(nv.NativeError, match="one utterance"):
            calls["fwd2_persistent"]()
        calls["fwd2_batch_persistent"]()
        calls["bwd2_batch_persistent"]()
    finally:
        nv.set_validate_only(False)
