"""A plain restatement of ``nn.LSTM(bidirectional=True)`` over a packed ragged batch, for the encoder bi-LSTM kernel tests.

One loop per utterance and direction, nothing batched, nothing shared with ``tacotron2_amd`` or the reference project: the
recurrence is written down once more from the definition of the operation, so that an error common to every native form
(launch chain, persistent launches) cannot hide behind their agreement with each other.  Dtype-generic: float64 is the
reference, float32 -- the same loop, the same order of operations -- is the yardstick for what sequential float32 arithmetic
costs on the very inputs of a test.

Inputs (per direction d):
  GX[d]   [B][T][4H]  the hoisted x . W_ih^T + b_ih + b_hh
  Whh[d]  [4H][H]
  lens    B lengths, 1 <= len <= T, in any order
  dout    [B][T][ndir * H]  (backward only)
Conventions: gate order i, f, g, o as in nn.LSTM; zero initial state; a direction with ``reverse`` set starts at each utterance's
OWN last frame and walks to frame 0.  Frames behind an utterance's length are never read and come out as zeros.

Layouts of what comes back are the ones ``t2amd_lstm_seq`` documents (include/tacotron2_amd.h): out [B][T][ndir * H], activated
gates [B][T][4H], cell states [T][B][H], DG [B][T][4H] = d sum(out * dout) / d GX by autograd on the loop itself.
"""
import torch


class BiLstmRef:
    """out [B][T][ndir H]; gates[d] [B][T][4H]; C[d] [T][B][H]; DG[d] [B][T][4H] (None without dout)."""

    def __init__(self, out, gates, C, DG):
        self.out, self.gates, self.C, self.DG = out, gates, C, DG


def _direction(GX, Whh, lens, reverse):
    B, T, H4 = GX.shape
    H = H4 // 4
    zero_h, zero_g = GX.new_zeros(H), GX.new_zeros(H4)
    outs, gates, cells = [], [], []
    for b in range(B):
        n = int(lens[b])
        assert 1 <= n <= T
        h, c = zero_h, zero_h
        o_t, g_t, c_t = [zero_h] * T, [zero_g] * T, [zero_h] * T
        for s in range(n):
            t = n - 1 - s if reverse else s
            pre = GX[b, t] + Whh @ h
            gi, gf = torch.sigmoid(pre[:H]), torch.sigmoid(pre[H:2 * H])
            gg, go = torch.tanh(pre[2 * H:3 * H]), torch.sigmoid(pre[3 * H:])
            c = gf * c + gi * gg
            h = go * torch.tanh(c)
            o_t[t], g_t[t], c_t[t] = h, torch.cat((gi, gf, gg, go)), c
        outs.append(torch.stack(o_t))
        gates.append(torch.stack(g_t))
        cells.append(torch.stack(c_t))
    return torch.stack(outs), torch.stack(gates), torch.stack(cells, dim=1)


def bilstm(GX, Whh, lens, dout=None, reverse=(0, 1), dtype=torch.float64):
    """GX / Whh: one tensor per direction (``reverse`` gives each direction's sense: (0, 1) is nn.LSTM's pair, (1,) a lone
    reverse direction).  Everything is computed in ``dtype`` on the CPU and returned detached, in ``dtype``."""
    assert len(GX) == len(Whh) == len(reverse)
    lens = [int(v) for v in lens]
    gx = [g.detach().to("cpu", dtype).clone().requires_grad_(dout is not None) for g in GX]
    w = [x.detach().to("cpu", dtype) for x in Whh]
    per_dir = [_direction(gx[d], w[d], lens, bool(reverse[d])) for d in range(len(gx))]
    out = torch.cat([p[0] for p in per_dir], dim=2)
    DG = None
    if dout is not None:
        (out * dout.detach().to("cpu", dtype)).sum().backward()
        DG = [g.grad.detach() if g.grad is not None else torch.zeros_like(g) for g in gx]
    return BiLstmRef(out.detach(), [p[1].detach() for p in per_dir], [p[2].detach() for p in per_dir], DG)


def weight_readings(DG, out_d, lens, reverse):
    """What the weight-gradient GEMMs downstream form from one direction's DG [B][T][4H]: dW_hh = sum_t DG_t^T . h_(t-1)
    ([4H][H]; h_(t-1) = the direction's own output one step earlier in ITS processing order, zero at its first step) and the
    bias gradient = the column sums of DG.  Float64, whatever comes in."""
    DG, out_d = DG.double(), out_d.double()
    B, T, H4 = DG.shape
    dW = DG.new_zeros(H4, H4 // 4)
    for b in range(B):
        n = int(lens[b])
        if n > 1:
            if reverse:
                dW += DG[b, :n - 1].t() @ out_d[b, 1:n]
            else:
                dW += DG[b, 1:n].t() @ out_d[b, :n - 1]
    return dW, DG.sum(dim=(0, 1))


def torch_bilstm(GX, Whh, lens, dout):
    """The operation itself: float64 ``torch.nn.LSTM(bidirectional=True, batch_first=True)`` under
    ``pack_padded_sequence(enforce_sorted=False)``.  nn.LSTM projects ONE input for both directions, so it is fed
    x = [GX[0] | GX[1]] with W_ih = [I 0] / [0 I] and zero biases: x . W_ih^T is then GX[d] exactly and d loss / d x is DG.
    -> (out [B][T][2H], [DG0, DG1], [dW_hh0, dW_hh1], [dbias0, dbias1]) for loss = sum(out * dout)."""
    B, T, H4 = GX[0].shape
    H = H4 // 4
    lstm = torch.nn.LSTM(2 * H4, H, num_layers=1, batch_first=True, bidirectional=True).double()
    eye, zero = torch.eye(H4, dtype=torch.float64), torch.zeros(H4, H4, dtype=torch.float64)
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.cat((eye, zero), dim=1))
        lstm.weight_ih_l0_reverse.copy_(torch.cat((zero, eye), dim=1))
        lstm.weight_hh_l0.copy_(Whh[0].double())
        lstm.weight_hh_l0_reverse.copy_(Whh[1].double())
        for nm in ("bias_ih_l0", "bias_hh_l0", "bias_ih_l0_reverse", "bias_hh_l0_reverse"):
            getattr(lstm, nm).zero_()
    x = torch.cat((GX[0].double(), GX[1].double()), dim=2).clone().requires_grad_(True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(x, torch.tensor([int(v) for v in lens]), batch_first=True, enforce_sorted=False)
    y, _ = lstm(packed)
    out, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True, total_length=T)
    (out * dout.double()).sum().backward()
    return (out.detach(), [x.grad[:, :, :H4].clone(), x.grad[:, :, H4:].clone()],
            [lstm.weight_hh_l0.grad.clone(), lstm.weight_hh_l0_reverse.grad.clone()],
            [lstm.bias_ih_l0.grad.clone(), lstm.bias_ih_l0_reverse.grad.clone()])


def lengths(pattern, B, T, g):
    """The three lengths patterns of the kernel tests, drawn from generator ``g``; max(lens) == T in all of them.
    sorted: descending, as the training batches come.  unsorted: a fixed permutation of the sorted draw (reversed, then
    neighbours swapped).  edge: at least one length 1, one length T and two equal neighbours (as far as B allows)."""
    lens = torch.randint(max(1, T // 3), T + 1, (B,), generator=g).sort(descending=True)[0]
    lens[0] = T
    if pattern == "sorted":
        return lens.tolist()
    if pattern == "unsorted":
        v = lens.flip(0).tolist()
        for i in range(0, B - 1, 2):
            v[i], v[i + 1] = v[i + 1], v[i]
        return v
    assert pattern == "edge"
    v = lens.tolist()
    if B >= 2:
        v[B // 2] = 1
    if B >= 4:
        v[1] = T                        # one more full-length row, not in front
        v[-1] = v[-2] = max(1, T // 2)  # two equal neighbours
    return v
