"""The small-batch kernels' restatement (tests/small_batch_ref.py) without a GPU: the float64 definition against torch.nn.LSTMCell
and F.linear in float64 on the same weights (gate order, bias, absent segments as zeros, the ``lens`` rule, the keep mask), the
float32 restatement against the float64 one, the NaN layout of the runners, what native.lstm_step_fwd puts into the C structure
for every ``bf16`` value, and the refusals of the two C entries in validate-only form."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fft_block_ref as fr
import small_batch_ref as sb
from tacotron2_amd import native

CPU = torch.device("cpu")
F32 = np.float32


def _cell(case):
    """torch.nn.LSTMCell in float64 holding the case's weights: segment 0 is its input, segment 1 its hidden state."""
    H, (w0, w1) = case["H"], case["widths"][:2]
    cell = torch.nn.LSTMCell(w0, H, bias=True).double()
    W = torch.from_numpy(case["W"]).double()
    with torch.no_grad():
        cell.weight_ih.copy_(W[:, :w0])
        cell.weight_hh.copy_(W[:, w0:w0 + w1])
        cell.bias_ih.copy_(torch.from_numpy(case["bias"]).double())
        cell.bias_hh.zero_()
    return cell


def _close(got, want):
    return np.abs(np.asarray(got) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("fmt", sb.FORMATS)
@pytest.mark.parametrize("B", [1, 3, 8])
def test_float64_definition_equals_torch_lstm_cell(B, fmt):
    """Two segments (input, hidden state), bias, c_prev; the gates are read back through h = o tanh(c) and c, and directly from
    the cell's own pre-activations in torch's order i, f, g, o."""
    case = sb.lstm_case(B, 12, (8, 12), fmt, gin=False)
    cell = _cell(case)
    x, h0 = (torch.from_numpy(a).double() for a in case["xs"])
    c0 = torch.from_numpy(case["c_prev"]).double()
    with torch.no_grad():
        h1, c1 = cell(x, (h0, c0))
        pre = F.linear(x, cell.weight_ih, cell.bias_ih) + F.linear(h0, cell.weight_hh)
    i, f, g, o = pre.chunk(4, dim=1)
    gates = torch.cat((torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)), dim=1)
    assert _close(h1, case["f64"]["h"]) and _close(c1, case["f64"]["c"]) and _close(gates, case["f64"]["gates"])
    assert np.abs(case["f64"]["h"]).max() > 0.05


def test_a_third_segment_equals_its_product_passed_as_gin():
    """pre = X W^T + gin + bias: a third segment's contribution, computed apart and passed as gin, gives the same step."""
    case = sb.lstm_case(3, 8, (8, 12, 16), gin=False)
    W = case["W"].astype(np.float64)
    gin = case["xs"][2].astype(np.float64) @ W[:, 20:].T
    two = sb.lstm_step64(case["xs"][:2], (8, 12), W[:, :20], 8, 3, gin=gin, bias=case["bias"], c_prev=case["c_prev"])
    for n in ("gates", "c", "h"):
        assert _close(two[n], case["f64"][n]), n


@pytest.mark.parametrize("absent", [0, 1, 2])
def test_an_absent_segment_is_a_segment_of_zeros(absent):
    case = sb.lstm_case(3, 8, (8, 16, 8), absent=(absent,))
    xs = [np.zeros((3, w), F32) if x is None else x for x, w in zip(case["xs"], case["widths"])]
    full = sb.lstm_step64(xs, case["widths"], case["W"], 8, 3, case["gin"], case["bias"], case["c_prev"])
    for n in ("gates", "c", "h"):
        assert np.array_equal(full[n], case["f64"][n]), n
    if absent == 1:                                                         # the hidden state of an LSTMCell at zero
        two = sb.lstm_case(2, 12, (8, 12), absent=(1,), gin=False)
        with torch.no_grad():
            h1, c1 = _cell(two)(torch.from_numpy(two["xs"][0]).double(), (torch.zeros(2, 12).double(), torch.from_numpy(two["c_prev"]).double()))
        assert _close(h1, two["f64"]["h"]) and _close(c1, two["f64"]["c"])


def test_optional_terms_absent_are_zero_terms():
    base = sb.lstm_case(2, 8, (8, 16, 8))
    for name in ("gin", "bias", "c_prev"):
        case = sb.lstm_case(2, 8, (8, 16, 8), **{name: False})
        assert case[name] is None
        kw = {n: case[n] for n in ("gin", "bias", "c_prev")}
        kw[name] = np.zeros_like(base[name])
        full = sb.lstm_step64(case["xs"], case["widths"], case["W"], 8, 2, **kw)
        for n in ("gates", "c", "h"):
            assert _close(full[n], case["f64"][n]), (name, n)


def test_rows_past_their_length_are_zero_and_the_others_unchanged():
    lens, t = (5, 2, 3, 9, 0), 2
    case = sb.lstm_case(5, 8, (8, 16, 8), lens=lens, t=t)
    free = sb.lstm_case(5, 8, (8, 16, 8))
    for n in ("gates", "c", "h"):
        for b, L in enumerate(lens):
            if t >= L:
                assert not case["f64"][n][b].any() and not sb.bits(case["f32"][n][b]).any(), (n, b)
            else:
                assert np.array_equal(case["f64"][n][b], free["f64"][n][b]), (n, b)
    assert [t >= L for L in lens] == [False, True, False, False, True]


def test_keep_mask_scales_h_alone():
    case, free = sb.lstm_case(4, 12, (8, 16, 8), keep=True), sb.lstm_case(4, 12, (8, 16, 8))
    assert case["keep_scale"] == native.scale_for(0.1) and 0 < case["keep"].sum() < case["keep"].size
    assert np.array_equal(case["f64"]["c"], free["f64"]["c"]) and np.array_equal(case["f64"]["gates"], free["f64"]["gates"])
    assert _close(case["f64"]["h"], free["f64"]["h"] * case["keep"] * float(np.float32(1.0) / np.float32(0.9)))


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("bias", [False, True])
def test_float64_linear_equals_torch_linear(act, bias):
    case = sb.linear_case(7, 17, 80, act, bias, keep=True)
    y = F.linear(torch.from_numpy(case["X"]).double(), torch.from_numpy(case["W"]).double(),
                 torch.from_numpy(case["bias"]).double() if bias else None)
    y = (F.relu(y) if act else y) * torch.from_numpy(case["keep"]).double() * case["keep_scale"]
    assert _close(y, case["f64"])
    assert (case["f64"] < 0).any() != bool(act)


def test_float32_restatements_lie_close_to_float64_and_bf16_weights_are_exact_in_bf16():
    for fmt in sb.FORMATS:
        case = sb.lstm_case(3, 8, sb.edge_widths(129, fmt), fmt)
        for n in ("gates", "c", "h"):
            assert case["f32"][n].dtype == F32 and case["f64"][n].dtype == np.float64
            assert 0 < fr.error(case["f32"][n], case["f64"][n]) < 64 * fr.U * max(1.0, np.abs(case["f64"][n]).max()), (fmt, n)
    assert np.array_equal(sb.bf16_round(case["W"]), case["W"]) and not (sb.bits(case["W"]) & 0xffff).any()
    lin = sb.linear_case(8, 81, 516)
    assert lin["f32"].dtype == F32 and 0 < fr.error(lin["f32"], lin["f64"]) < 64 * fr.U * np.abs(lin["f64"]).max()


def test_loop_edge_widths_add_up_and_keep_the_segment_rules():
    for fmt in sb.FORMATS:
        for Kn in sb.LOOP_EDGES:
            widths = sb.edge_widths(Kn, fmt)
            assert sum(widths) == (8 if fmt == "bf16" else 4) * Kn and all(w > 0 and w % 4 == 0 for w in widths), (fmt, Kn)
            assert len(widths) == 3 or sum(widths) < 12
    assert sb.edge_widths(65, "bf16")[:2] == (12, 20) and sb.edge_widths(129, "bf16")[:2] == (12, 20)


def test_planted_biases_saturate_as_the_constants_say():
    case = sb.lstm_case(3, 8, (8, 16, 8), planted=True, quiet=0.25)
    pre, H = case["f64"]["pre"], 8
    assert np.abs(pre - case["bias"].astype(np.float64)).max() < 2.0       # 20 - 2 = SIGMOID_ONE, -100 + 2 < SIGMOID_ZERO
    g32 = case["f32"]["gates"]
    for g in range(4):
        cols = g32[:, g * H:g * H + 4]
        if g == 2:
            assert np.array_equal(cols, np.broadcast_to(np.asarray((1, -1, 1, -1), F32), cols.shape))
        else:
            assert (cols[:, (0, 2)] == 1).all() and not sb.bits(cols[:, 1]).any() and (cols[:, 3] > 0).all() and (cols[:, 3] < 1e-7).all()


def test_slab_lays_data_inside_nan_and_sees_a_write_beside_it():
    a = np.arange(6, dtype=F32).reshape(2, 3)
    s = sb.Slab(CPU, data=a, pad=5, lead=4)
    assert s.view.stride() == (8, 1) and s.view.data_ptr() - s.whole.data_ptr() == 16 and s.whole.numel() == 20
    assert np.array_equal(s.numpy(), a) and s.intact() and torch.isnan(s.whole).sum() == 14
    s.view[1, 2] = 7.0
    assert s.intact()
    s.whole[4 + 3] = 0.0
    assert not s.intact()
    w = sb.Slab(CPU, data=np.ones((4, 8), F32), pad=0, lead=8, dtype=torch.bfloat16)
    assert w.view.is_contiguous() and w.whole.numel() == 48 and w.intact()
    w.whole[-1] = 0.0
    assert not w.intact()


class _Recorder:
    """Stands for the library: keeps a copy of the structure that native.lstm_step_fwd filled."""

    def _take(self, ref, stream):
        self.step = native.LstmStep.from_buffer_copy(ref._obj)
        return 0

    t2amd_lstm_step_small_f32 = t2amd_lstm_step_fwd_f32 = _take


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(native, "_lib", rec)
    monkeypatch.setattr(native, "_validate_only", True)                     # host pointers pass
    return rec


def test_lstm_step_fwd_fills_the_structure_for_every_bf16_value(recorder):
    B, H, K = 2, 8, 16
    f32 = lambda *s: torch.zeros(*s)                                        # noqa: E731
    b16 = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)                  # noqa: E731
    gates, c, h = f32(B, 4 * H), f32(B, H), f32(B, H)
    for small in (False, True):
        native.lstm_step_fwd([f32(B, K)], [K], f32(4 * H, K), H, B, gates, c, h, small=small)
        s = recorder.step
        assert (s.bf16, s.gates_out, s.ld_gates, s.c_out, s.h_out) == (0, gates.data_ptr(), 4 * H, c.data_ptr(), h.data_ptr())
        native.lstm_step_fwd([b16(B, K)], [K], b16(4 * H, K), H, B, gates, c, h, small=small, bf16=True)
        assert recorder.step.bf16 == 1
        native.lstm_step_fwd([b16(B, 2 * K)], [K], b16(4 * H, 2 * K), H, B, gates, c, h, small=small, bf16=3)
        assert recorder.step.bf16 == 3 and recorder.step.x[0].ld == K
    W = b16(4 * H, K)
    native.lstm_step_fwd([f32(B, K)], [K], W, H, B, None, c, h, small=True, bf16=2)
    s = recorder.step
    assert (s.bf16, s.W, s.gates_out, s.ld_gates, s.Ktot) == (2, W.data_ptr(), None, 0, K)
    with pytest.raises(native.NativeError):                                 # bf16 weights, f32 inputs: nothing else
        native.lstm_step_fwd([b16(B, K)], [K], W, H, B, None, c, h, small=True, bf16=2)
    with pytest.raises(native.NativeError):
        native.lstm_step_fwd([f32(B, K)], [K], f32(4 * H, K), H, B, None, c, h, small=True, bf16=2)


@pytest.mark.parametrize("name,call", sb.refusals(), ids=[n.replace(" ", "_") for n, _ in sb.refusals()])
def test_the_entries_refuse_in_validate_only_form(native_lib, name, call):
    native.set_validate_only(True)
    try:
        with pytest.raises(native.NativeError):
            call(CPU)
    finally:
        native.set_validate_only(False)


def test_the_entries_accept_the_largest_case_in_validate_only_form(native_lib):
    """B = 8 with K = 5088 is 163,328 bytes of LDS, 512 under the limit that K = 5120 exceeds."""
    native.set_validate_only(True)
    try:
        for fmt in sb.FORMATS:
            case = dict(B=8, H=4, widths=(2048, 1024, 2016), fmt=fmt, W=np.zeros((16, 5088), F32), t=0, keep_scale=1.0,
                        xs=[np.zeros((8, w), F32) for w in (2048, 1024, 2016)], gin=None, bias=None, c_prev=None, keep=None, lens=None)
            out = sb.run_lstm(case, CPU)
            assert np.isnan(out["c"]).all()                                 # nothing ran
    finally:
        native.set_validate_only(False)
