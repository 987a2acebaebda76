"""The small-batch (B <= 8) matrix-vector kernels of csrc/gemv.hip on the MI355X (native.lstm_step_fwd(small=True) with f32 and
with bf16 weights, native.linear_small) against the float64 restatement (tests/small_batch_ref.py).

Per case and per tensor the largest absolute error is at most
max(4 x the float32 restatement's own largest error on that case, 8 2^-24 max(1, largest |value| of that tensor in float64))
("Tolerance of the small-batch kernels").  Every tensor lies inside a wider buffer of NaN, and what
surrounds an output must still be NaN after the call.  Every case prints its ratios error / allowed (``FIGURE`` lines;
profiles/small_batch_pytest_gpu.txt has the run)."""
import numpy as np
import pytest
import torch

import small_batch_ref as sb
from tacotron2_amd import native

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
WIDTHS = (8, 16, 8)
LDS_WIDTHS = (1024, 512, 1024)                                   # B = 8: 4 (8 x 2560 + 16 x 8) = 82,432 bytes of LDS


# ---- the LSTM form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", sb.FORMATS)
@pytest.mark.parametrize("B", sb.EVERY_B)
def test_lstm_every_batch_size_on_three_workgroups(native_lib, B, fmt):
    """H = 12 is three workgroups and no multiple of 16; K = 32 is 8 (4) sixteen-byte units a row: most lanes hold nothing.  The
    rows from B up to the next power of two are staged as zeros."""
    case = sb.lstm_case(B, 12, WIDTHS, fmt)
    sb.check_lstm(case, sb.run_lstm(case, DEV), "every B ")


@pytest.mark.parametrize("fmt", sb.FORMATS)
@pytest.mark.parametrize("Kn", sb.LOOP_EDGES)
def test_lstm_loop_edges(native_lib, Kn, fmt):
    """Kn sixteen-byte units a weight row: the two-pieces-in-flight loop takes k, k + 64 while k + 64 < Kn, the tail the rest."""
    case = sb.lstm_case(3, 8, sb.edge_widths(Kn, fmt), fmt)
    sb.check_lstm(case, sb.run_lstm(case, DEV), "Kn %d " % Kn)


@pytest.mark.parametrize("fmt", sb.FORMATS)
@pytest.mark.parametrize("absent", [0, 1, 2])
def test_lstm_absent_segment(native_lib, absent, fmt):
    case = sb.lstm_case(3, 12, WIDTHS, fmt, absent=(absent,))
    sb.check_lstm(case, sb.run_lstm(case, DEV), "absent %d " % absent)


@pytest.mark.parametrize("fmt", sb.FORMATS)
@pytest.mark.parametrize("without", ["gin", "bias", "c_prev", "gates_out"])
def test_lstm_optional_arguments(native_lib, without, fmt):
    """gin, bias and c_prev absent in turn; without gates_out, c and h are the bits of the call that writes the gates."""
    if without == "gates_out":
        case = sb.lstm_case(5, 12, WIDTHS, fmt)
        out, full = sb.run_lstm(case, DEV, gates=False), sb.run_lstm(case, DEV)
        assert out["gates"] is None and all(np.array_equal(sb.bits(out[n]), sb.bits(full[n])) for n in ("c", "h"))
    else:
        case = sb.lstm_case(5, 12, WIDTHS, fmt, **{without: False})
        out = sb.run_lstm(case, DEV)
    sb.check_lstm(case, out, "no %s " % without)


@pytest.mark.parametrize("fmt", sb.FORMATS)
def test_lstm_keep_mask(native_lib, fmt):
    """Keep rate 0.9, keep_scale = scale_for(0.1): a dropped unit's h is exact +0, its c and gates are not touched by the mask."""
    case = sb.lstm_case(6, 12, WIDTHS, fmt, keep=True)
    out = sb.run_lstm(case, DEV)
    sb.check_lstm(case, out, "keep ")
    dropped = case["keep"] == 0
    assert dropped.any() and not sb.bits(out["h"][dropped]).any() and (out["c"][dropped] != 0).all()


@pytest.mark.parametrize("fmt", sb.FORMATS)
def test_lstm_rows_past_their_length_are_exact_zero(native_lib, fmt):
    lens, t = (5, 2, 3, 9, 0, 3, 2), 2
    case = sb.lstm_case(7, 12, WIDTHS, fmt, keep=True, lens=lens, t=t)
    out = sb.run_lstm(case, DEV)
    sb.check_lstm(case, out, "lens ")                                       # asserts the bit-exact +0 rows
    past = np.asarray(lens) <= t
    assert past.sum() == 3 and all(not sb.bits(out[n][past]).any() and out[n][~past].any(axis=1).all() for n in ("gates", "c", "h"))


@pytest.mark.parametrize("fmt", sb.FORMATS)
def test_lstm_saturation(native_lib, fmt):
    """Biases of +-100 and +-20 on units 0 .. 3 of every gate: exact 0 / 1 / +-1 wherever float32 saturates (the thresholds of
    small_batch_ref), everything finite, and the tolerance against float64 as everywhere."""
    case = sb.lstm_case(3, 8, WIDTHS, fmt, planted=True, quiet=0.25)
    out = sb.run_lstm(case, DEV)
    sb.check_lstm(case, out, "planted ")
    H, pre, gates = 8, case["f64"]["pre"], out["gates"]
    for g in (0, 1, 3):
        p, v = pre[:, g * H:(g + 1) * H], gates[:, g * H:(g + 1) * H]
        one, zero = p >= sb.SIGMOID_ONE, p <= sb.SIGMOID_ZERO
        assert one.sum() == 6 and zero.sum() == 3, (g, one.sum(), zero.sum())
        assert (v[one] == 1).all() and not sb.bits(v[zero]).any(), g
        assert ((v >= 0) & (v <= 1)).all()
    p, v = pre[:, 2 * H:3 * H], gates[:, 2 * H:3 * H]
    sat = np.abs(p) >= sb.TANH_ONE
    assert sat.sum() == 12 and np.array_equal(v[sat], np.sign(p[sat]).astype(np.float32))
    assert np.isfinite(out["c"]).all() and np.isfinite(out["h"]).all() and (np.abs(out["h"]) <= 1).all()


@pytest.mark.parametrize("fmt", sb.FORMATS)
@pytest.mark.parametrize("B", [5, 8])
def test_lstm_row_of_a_batch_equals_that_row_alone(native_lib, B, fmt):
    """A lane's k order and the wave reduction are the same in every NB instantiation: bit for bit."""
    case = sb.lstm_case(B, 12, WIDTHS, fmt, keep=True)
    out = sb.run_lstm(case, DEV)
    sb.check_lstm(case, out, "rows alone ")
    for b in range(B):
        alone = sb.run_lstm(sb.lstm_row(case, b), DEV)
        for n in ("gates", "c", "h"):
            assert np.array_equal(sb.bits(out[n][b]), sb.bits(alone[n][0])), (b, n)


def test_lstm_matrix_vector_and_mfma_forms_agree(native_lib):
    """f32 weights, an absent middle segment, bias alone: the assertion of test_kernels_gpu.py's small-batch test, and the
    matrix-vector form under the tolerance."""
    case = sb.lstm_case(3, 256, (256, 512, 64), absent=(1,), gin=False, c_prev=False)
    small = sb.run_lstm(case, DEV)
    sb.check_lstm(case, small, "both forms ")
    mfma = sb.run_lstm(case, DEV, small=False, pad=0)
    for n in ("gates", "h"):
        assert np.abs(small[n] - mfma[n]).max() / max(1.0, np.abs(mfma[n]).max()) < 1e-5, n


@pytest.mark.parametrize("fmt", sb.FORMATS)
def test_lstm_above_64_kib_of_lds(native_lib, fmt):
    case = sb.lstm_case(8, 4, LDS_WIDTHS, fmt)
    sb.check_lstm(case, sb.run_lstm(case, DEV), "82,432 bytes of LDS ")


# ---- the linear form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", sb.LIN_B)
@pytest.mark.parametrize("N", sb.LIN_N)
def test_linear_shapes(native_lib, N, B):
    """Every K and both activations at this (N, B); the weight rows lie K + 4 apart."""
    for K in sb.LIN_K:
        for act in (0, 1):
            case = sb.linear_case(B, N, K, act)
            sb.check_linear(case, sb.run_linear(case, DEV))


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("bias", [False, True])
def test_linear_keep_mask_and_absent_bias(native_lib, bias, act):
    for B, N, K in ((7, 17, 260), (4, 81, 80)):
        case = sb.linear_case(B, N, K, act, bias, keep=True)
        y = sb.run_linear(case, DEV)
        sb.check_linear(case, y, "keep ")
        assert not sb.bits(y[case["keep"] == 0]).any()
        case = sb.linear_case(B, N, K, act, bias)
        sb.check_linear(case, sb.run_linear(case, DEV))


@pytest.mark.parametrize("B", sb.LIN_B)
def test_linear_scalar_staging_equals_float4_staging(native_lib, B):
    """Rows 81 floats apart from a base one float into the buffer (the projection slab's layout) take the scalar staging loop:
    the same bits as the float4 loop on the same values."""
    case = sb.linear_case(B, 81, 80, 1, keep=True)
    vec = sb.run_linear(case, DEV)
    scalar = sb.run_linear(case, DEV, x_pad=1, x_lead=1)
    sb.check_linear(case, scalar, "ldx 81, base 4 bytes in ")
    assert np.array_equal(sb.bits(vec), sb.bits(scalar))


# ---- refusals and the launch order -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,call", sb.refusals(), ids=[n.replace(" ", "_") for n, _ in sb.refusals()])
def test_refusals_launch_nothing(native_lib, name, call):
    """NativeError, and the outputs are still NaN everywhere (checked by the runners before they pass the error on)."""
    with pytest.raises(native.NativeError):
        call(DEV)


def test_more_than_64_kib_in_a_second_instantiation_after_a_larger_first(native_lib):
    """small_launch keeps one high-water mark of the dynamic LDS it has asked for and raises a kernel's limit only above it: after
    the LSTM form at B = 8, K = 2560 (82,432 bytes, <true, 8>) the linear form at B = 3, K = 4352 (69,888 bytes, <false, 4>) is
    launched without its own limit ever having been raised.  Observed on the MI355X: the runtime accepts that launch and both
    results are within the tolerance; a refusal would show as a NativeError from the launch check."""
    for fmt in sb.FORMATS:
        first = sb.lstm_case(8, 4, LDS_WIDTHS, fmt)
        sb.check_lstm(first, sb.run_lstm(first, DEV), "launch order, first ")
    second = sb.linear_case(3, 16, 4352)
    assert 4 * (4 * 4352 + 16 * 4) == 69888
    sb.check_linear(second, sb.run_linear(second, DEV), "launch order, second ")
