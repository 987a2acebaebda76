"""The five native forms of the encoder bi-LSTM against a float64 restatement of nn.LSTM(bidirectional=True) over a packed
ragged batch (tests/bilstm_ref.py, itself pinned to torch.nn.LSTM by tests/test_bilstm_ref_cpu.py).

Forms: the launch chains t2amd_lstm_seq_{fwd2,bwd2}_f32 (csrc/loops.hip; both directions, and one direction with q == NULL),
the one-utterance persistent forward, the batch-persistent forward and the batch-persistent BPTT (csrc/decode_persist.hip).
test_zz7 compares them with each other; here every output is held to the operation: h, the activated gates left in GX, the
cell states, the gate gradients DG, and -- for the chain backward -- the W_hh and bias gradients that follow from DG.

75 cases: 16 chain forward + backward (every H in 64..256 x every B in 1, 7, 33, 70; T in 1, 2, 23 and the three lengths
patterns spread over them so that every T meets every pattern), 6 one-direction chain, 10 chain backward over dx_splits,
16 batch-persistent forward, 16 batch-persistent BPTT, 10 one-utterance persistent forward, 1 weight-gradient reading.
All draws are made on the CPU with a seeded generator; GX and dout hold ordinary random values behind every utterance's length
(the kernels must ignore them) and every buffer a call writes starts NaN-filled.  References are computed once per drawn case
and shared between the forms.

Tolerances.  The chains and the two persistent forwards are exact f32: they differ from a sequential float32 evaluation only in
summation order over K = H <= 256 (and in the last bits of sigmoid / tanh).  The yardstick is therefore the SAME restatement run
in float32 on the CPU: per tensor e32 = max|ref32 - ref64|, and the assertion is
    max|kernel - ref64| <= R * e32 + 1e-7 * max|ref64|
(the floor covers tensors where the float32 run happens to be exact, e.g. T = 1 with zero initial state).  R = 3 x the worst
ratio measured on the MI355X, rounded up (the project's rule for measured gates).  Measured
(profiles/encoder_bilstm_ref_pytest_gpu.txt): every tensor of every exact-f32 form lies between 0.7 and 2.2 x e32 -- the
kernels are as close to float64 as sequential float32 is; worst 2.153 -> R = 7.
The batch-persistent BPTT forms its recurrent product in split-bf16 (three terms at ~2^-17 relative each): it keeps the project's
bound, now against float64: max|DG - DG_ref64| < 2e-5 * max|DG_ref64| (measured: at most 1.5e-6, 9 - 12 x e32).
Every figure is printed before it is asserted, and the table of worst ratios per form and tensor closes the run (pytest -s).
"""
import functools

import pytest
import torch

import bilstm_ref as br

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 7.0                      # 3 x 2.153 (batch-persistent forward, gates[0], H = 64 B = 33 T = 23 edge), rounded up
FLOOR = 1e-7
BPTT_PERSISTENT_REL = 2e-5   # include/tacotron2_amd.h: split-bf16 recurrent product
PATTERNS = ("sorted", "unsorted", "edge")

# every H meets every B; every T in (1, 2, 23) meets every lengths pattern
GRID = [(64, 1, 23, "sorted"), (64, 7, 2, "unsorted"), (64, 33, 23, "edge"), (64, 70, 1, "sorted"),
        (128, 1, 2, "sorted"), (128, 7, 23, "unsorted"), (128, 33, 1, "edge"), (128, 70, 2, "edge"),
        (192, 1, 1, "unsorted"), (192, 7, 23, "edge"), (192, 33, 2, "sorted"), (192, 70, 2, "unsorted"),
        (256, 1, 23, "unsorted"), (256, 7, 1, "edge"), (256, 33, 23, "sorted"), (256, 70, 23, "edge")]
ONE_DIRECTION = [(64, 0, "sorted"), (64, 1, "unsorted"), (64, 1, "edge"), (192, 0, "unsorted"), (192, 0, "edge"), (192, 1, "sorted")]
DX_SPLITS = [(64, 0, 7, "sorted"), (64, 1, 33, "unsorted"), (64, 2, 7, "edge"), (64, 4, 33, "sorted"),
             (256, 0, 33, "unsorted"), (256, 1, 7, "edge"), (256, 2, 33, "edge"), (256, 4, 7, "unsorted"),
             (192, 3, 7, "sorted"), (192, 3, 33, "unsorted")]
ONE_UTTERANCE = [(64, 1), (64, 37), (128, 2), (128, 37), (192, 5), (192, 37), (256, 1), (256, 2), (256, 5), (256, 37)]

_rows = []


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    yield
    worst = {}
    for form, tensor, case, err, e32, scale in _rows:
        k = (form, tensor)
        ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
        w = worst.setdefault(k, dict(ratio=0.0, ratio_case="", rel=0.0, n=0))
        w["n"] += 1
        w["rel"] = max(w["rel"], err / scale if scale > 0 else 0.0)
        if e32 >= FLOOR * scale and ratio > w["ratio"]:           # (below the floor the ratio says nothing: the floor decides)
            w["ratio"], w["ratio_case"] = ratio, case
    print("\n# worst per form and tensor: max|kernel - ref64| / e32 over the cases with e32 >= 1e-7 max|ref64|, and max|kernel - ref64| / max|ref64|")
    for (form, tensor), w in sorted(worst.items()):
        print("%-28s %-8s cases %3d  worst ratio %8.3f (%s)  worst err/scale %.3e"
              % (form, tensor, w["n"], w["ratio"], w["ratio_case"], w["rel"]))


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(H, B, T, pattern):
    """One drawn problem (CPU, seeded) with its float64 reference and float32 yardstick; shared and never modified."""
    c = Case()
    c.H, c.B, c.T, c.pattern = H, B, T, pattern
    c.name = "H=%d B=%d T=%d %s" % (H, B, T, pattern)
    g = torch.Generator().manual_seed(100000 * PATTERNS.index(pattern) + 1000 * H + 10 * B + T)
    c.lens = br.lengths(pattern, B, T, g)
    assert max(c.lens) == T and min(c.lens) >= 1
    c.Whh = [torch.randn(4 * H, H, generator=g) * (H ** -0.5) for _ in range(2)]
    c.GX = [torch.randn(B, T, 4 * H, generator=g) * 0.7 for _ in range(2)]
    c.dout = torch.randn(B, T, 2 * H, generator=g) * 0.3
    c.ref64 = br.bilstm(c.GX, c.Whh, c.lens, c.dout)
    c.ref32 = br.bilstm(c.GX, c.Whh, c.lens, c.dout, dtype=torch.float32)
    c.valid = torch.arange(T).unsqueeze(0) < torch.tensor(c.lens).unsqueeze(1)           # [B][T]
    return c


def _compare(form, tensor, c, got, ref64, ref32, failures, rel=None):
    """Record and print the figures of one tensor, then judge it (failures are collected so that every figure is seen)."""
    got, ref32 = got.double(), ref32.double()
    if not bool(torch.isfinite(got).all()):
        failures.append("%s %s %s: %d non-finite values left in the written region" % (form, tensor, c.name, int((~torch.isfinite(got)).sum())))
        return
    err, e32, scale = float((got - ref64).abs().max()), float((ref32 - ref64).abs().max()), float(ref64.abs().max())
    _rows.append((form, tensor, c.name, err, e32, scale))
    bound = rel * scale if rel is not None else R * e32 + FLOOR * scale
    print("%s %s %s: err %.3e e32 %.3e scale %.3e bound %.3e" % (form, tensor, c.name, err, e32, scale, bound))
    if rel is not None:
        if not err < bound:
            failures.append("%s %s %s: err %.3e >= %g * %.3e" % (form, tensor, c.name, err, rel, scale))
    elif not err <= bound:
        failures.append("%s %s %s: err %.3e > %g * e32 %.3e + %g * %.3e" % (form, tensor, c.name, err, R, e32, FLOOR, scale))


def _zero_behind(form, tensor, c, got_bt, failures):
    """got_bt [B][T][...]: exactly 0.0 behind every utterance's length."""
    tail = got_bt[~c.valid]
    if tail.numel() and not bool(torch.all(tail == 0.0)):
        failures.append("%s %s %s: %d values behind a length are not exactly 0" % (form, tensor, c.name, int((tail != 0.0).sum())))


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


class Run:
    """Device buffers and descriptors of one problem, directions ``dirs`` (a subset of (0, 1)) packed side by side."""

    def __init__(self, nv, c, dirs=(0, 1)):
        self.nv, self.c, self.dirs = nv, c, dirs
        B, T, H = c.B, c.T, c.H
        self.E = E = len(dirs) * H
        self.lens = torch.tensor(c.lens, dtype=torch.int32).to(DEV)
        self.Whh = [c.Whh[d].to(DEV) for d in dirs]
        self.WhhT = [w.t().contiguous() for w in self.Whh]
        self.GX = [c.GX[d].reshape(B * T, 4 * H).to(DEV) for d in dirs]           # overwritten with the activated gates
        self.mem, self.C = _nan(B, T, E), [_nan(T, B, H) for _ in dirs]
        self.dmem = torch.cat([c.dout[:, :, d * H:(d + 1) * H] for d in dirs], dim=2).contiguous().to(DEV)
        self.fwd = []
        for i, d in enumerate(dirs):
            desc = nv.LstmSeq()
            desc.B, desc.T, desc.H, desc.reverse = B, T, H, d
            desc.Whh, desc.GX = nv.ptr(self.Whh[i]), nv.ptr(self.GX[i])
            desc.out, desc.ld_out = nv.ptr(self.mem.view(B * T, E)[:, i * H:(i + 1) * H]), E
            desc.C, desc.lens = nv.ptr(self.C[i]), nv.ptr(self.lens, torch.int32)
            self.fwd.append(desc)

    def backward_descs(self, dx_splits):
        nv, c = self.nv, self.c
        B, T, H, E = c.B, c.T, c.H, self.E
        self.DG = [_nan(B * T, 4 * H) for _ in self.dirs]
        self.dX, self.dc = [_nan(max(dx_splits, 1), B, H) for _ in self.dirs], [_nan(B, H) for _ in self.dirs]
        bwd = []
        for i, d in enumerate(self.dirs):
            desc = nv.LstmSeq()
            desc.B, desc.T, desc.H, desc.reverse = B, T, H, d
            desc.WhhT = nv.ptr(self.WhhT[i])
            desc.GX, desc.C, desc.lens = nv.ptr(self.GX[i]), nv.ptr(self.C[i]), nv.ptr(self.lens, torch.int32)
            desc.dout, desc.ld_dout = nv.ptr(self.dmem.view(B * T, E)[:, i * H:(i + 1) * H]), E
            desc.DG = nv.ptr(self.DG[i])
            desc.dX, desc.dc, desc.dx_splits = nv.ptr(self.dX[i]), nv.ptr(self.dc[i]), dx_splits
            bwd.append(desc)
        return bwd

    def chain_forward(self):
        if len(self.dirs) == 2:
            self.nv.lstm_seq_fwd2(self.fwd[0], self.fwd[1])
        else:
            self.nv.lstm_seq_fwd(self.fwd[0])
        torch.cuda.synchronize()

    def chain_backward(self, dx_splits):
        bwd = self.backward_descs(dx_splits)
        if len(self.dirs) == 2:
            self.nv.lstm_seq_bwd2(bwd[0], bwd[1])
        else:
            self.nv.lstm_seq_bwd(bwd[0])
        torch.cuda.synchronize()

    def check_forward(self, form, failures, state=True):
        c, H = self.c, self.c.H
        mem = self.mem.cpu()
        for i, d in enumerate(self.dirs):
            sl = slice(d * H, (d + 1) * H)
            _compare(form, "out[%d]" % d, c, mem[:, :, i * H:(i + 1) * H], c.ref64.out[:, :, sl], c.ref32.out[:, :, sl], failures)
            if state:
                gates, cell = self.GX[i].cpu().view(c.B, c.T, 4 * H), self.C[i].cpu()
                _compare(form, "gates[%d]" % d, c, gates, c.ref64.gates[d], c.ref32.gates[d], failures)
                _compare(form, "C[%d]" % d, c, cell, c.ref64.C[d], c.ref32.C[d], failures)
                _zero_behind(form, "gates[%d]" % d, c, gates, failures)
                _zero_behind(form, "C[%d]" % d, c, cell.transpose(0, 1), failures)
        _zero_behind(form, "out", c, mem, failures)

    def check_backward(self, form, failures, rel=None):
        c = self.c
        for i, d in enumerate(self.dirs):
            DG = self.DG[i].cpu().view(c.B, c.T, 4 * c.H)
            _compare(form, "DG[%d]" % d, c, DG, c.ref64.DG[d], c.ref32.DG[d], failures, rel=rel)
            _zero_behind(form, "DG[%d]" % d, c, DG, failures)


def _persistent_or_skip(c, why):
    """A _supported refusal on the machine's CU count may skip the B = 70, H = 256 case only; it is never routed to the chain."""
    if why is None:
        return
    if (c.B, c.H) == (70, 256) and "co-resident" in why:
        pytest.skip(why)
    pytest.fail("%s: refused where it must run: %s" % (c.name, why))


def _status_ok(nv, status, what):
    if int(status.item()) != 0:
        pytest.fail("%s gave up (status %d); encoder_handoff_timeouts() = %d" % (what, int(status.item()), nv.encoder_handoff_timeouts()))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("H,B,T,pattern", GRID)
def test_chain_forward_and_backward_against_float64(native_lib, H, B, T, pattern):
    """t2amd_lstm_seq_fwd2_f32 then t2amd_lstm_seq_bwd2_f32 (dx_splits = 4, what the engine runs) on its own forward state."""
    from tacotron2_amd import native as nv
    c, failures = _case(H, B, T, pattern), []
    run = Run(nv, c)
    run.chain_forward()
    run.check_forward("chain fwd2", failures)
    run.chain_backward(4)
    run.check_backward("chain bwd2", failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("H,reverse,pattern", ONE_DIRECTION)
def test_chain_one_direction_against_float64(native_lib, H, reverse, pattern):
    """t2amd_lstm_seq_fwd_f32 / t2amd_lstm_seq_bwd_f32 (q == NULL), each sense alone: a lone reverse direction starts at each
    utterance's own last frame."""
    from tacotron2_amd import native as nv
    c, failures = _case(H, 7, 9, pattern), []
    run = Run(nv, c, dirs=(reverse,))
    run.chain_forward()
    run.check_forward("chain fwd one direction", failures)
    run.chain_backward(4 if H == 64 else 3)
    run.check_backward("chain bwd one direction", failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("H,dx_splits,B,pattern", DX_SPLITS)
def test_chain_backward_over_dx_splits_against_float64(native_lib, H, dx_splits, B, pattern):
    """The recurrent data-gradient product split over 0 / 1 (one slab), 2, 3 (legal at H = 192 only) and 4 groups of k tiles:
    the next step's cell backward adds that many partial slabs."""
    from tacotron2_amd import native as nv
    c, failures = _case(H, B, 9, pattern), []
    run = Run(nv, c)
    run.chain_forward()
    run.chain_backward(dx_splits)
    run.check_backward("chain bwd2 dx_splits=%d" % dx_splits, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("H,B,T,pattern", GRID)
def test_batch_persistent_forward_against_float64(native_lib, H, B, T, pattern):
    """t2amd_lstm_seq_fwd2_batch_persistent_f32: every fragment load is guarded by the width, so H < 256 runs other code than
    H = 256; B = 33 leaves a row group of one utterance, B = 70 one of six."""
    from tacotron2_amd import native as nv
    c, failures = _case(H, B, T, pattern), []
    run = Run(nv, c)
    _persistent_or_skip(c, nv.lstm_seq_batch_persistent_supported(run.fwd[0], 2, _cus()))
    flags = torch.full((nv.lstm_seq_batch_persistent_flag_words(B, H, 2),), 77, dtype=torch.int32, device=DEV)
    status, poison = torch.full((1,), 5, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV)
    nv.lstm_seq_fwd2_batch_persistent(run.fwd[0], run.fwd[1], flags, status, poison)
    torch.cuda.synchronize()
    _status_ok(nv, status, "batch-persistent forward " + c.name)
    run.check_forward("batch-persistent fwd", failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("H,B,T,pattern", GRID)
def test_batch_persistent_bptt_against_float64(native_lib, H, B, T, pattern):
    """t2amd_lstm_seq_bwd2_batch_persistent_f32 on the chain forward's state: the project's 2e-5 bound, against float64."""
    from tacotron2_amd import native as nv
    c, failures = _case(H, B, T, pattern), []
    run = Run(nv, c)
    run.chain_forward()
    bwd = run.backward_descs(4)
    _persistent_or_skip(c, nv.lstm_seq_bwd2_batch_persistent_supported(bwd[0], 2, _cus()))
    flags = torch.full((nv.lstm_seq_batch_persistent_flag_words(B, H, 2),), 77, dtype=torch.int32, device=DEV)
    status, poison = torch.full((1,), 5, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV)
    nv.lstm_seq_bwd2_batch_persistent(bwd[0], bwd[1], flags, status, poison)
    torch.cuda.synchronize()
    _status_ok(nv, status, "batch-persistent BPTT " + c.name)
    run.check_backward("batch-persistent bwd", failures, rel=BPTT_PERSISTENT_REL)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("H,T", ONE_UTTERANCE)
def test_one_utterance_persistent_forward_against_float64(native_lib, H, T):
    """t2amd_lstm_seq_fwd2_persistent_f32 (inference): writes `out` only -- GX must come back bit-identical, C is not its to write."""
    from tacotron2_amd import native as nv
    c, failures = _case(H, 1, T, "sorted"), []
    run = Run(nv, c)
    why = nv.lstm_seq_persistent_supported(run.fwd[0])
    assert why is None, why
    mailbox = torch.full((nv.load().t2amd_lstm_seq_persistent_mailbox_bytes(H, 2) // 8,), 77, dtype=torch.int64, device=DEV)
    status = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    nv.lstm_seq_fwd2_persistent(run.fwd[0], run.fwd[1], mailbox, status)
    torch.cuda.synchronize()
    _status_ok(nv, status, "one-utterance persistent forward " + c.name)
    run.check_forward("one-utterance persistent fwd", failures, state=False)
    for d in range(2):
        if not torch.equal(run.GX[d].cpu().view(1, T, 4 * H), c.GX[d]):
            failures.append("one-utterance persistent fwd %s: GX[%d] was modified" % (c.name, d))
    assert not failures, "\n".join(failures)


def test_chain_backward_gate_gradients_give_nn_lstm_weight_gradients(native_lib):
    """Two independent readings of the chain backward's DG, as the weight-gradient GEMMs downstream form them:
    dW_hh = sum_t DG_t^T . h_(t-1) (float64 on the host, from the kernel's DG and the reference h) and the column sums of DG,
    against autograd's W_hh and bias gradients of float64 nn.LSTM over the packed batch (H = 64, B = 7, T = 9, unsorted)."""
    from tacotron2_amd import native as nv
    H = 64
    c, failures = _case(H, 7, 9, "unsorted"), []
    _, _, dW, db = br.torch_bilstm(c.GX, c.Whh, c.lens, c.dout)
    run = Run(nv, c)
    run.chain_forward()
    run.chain_backward(4)
    for d in range(2):
        h64 = c.ref64.out[:, :, d * H:(d + 1) * H]
        gW, gb = br.weight_readings(run.DG[d].cpu().view(c.B, c.T, 4 * H), h64, c.lens, d)
        yW, yb = br.weight_readings(c.ref32.DG[d], h64, c.lens, d)        # the same readings of the float32 yardstick's DG
        _compare("chain bwd2 readings", "dW_hh[%d]" % d, c, gW, dW[d], yW, failures)
        _compare("chain bwd2 readings", "dbias[%d]" % d, c, gb, db[d], yb, failures)
    assert not failures, "\n".join(failures)
