"""The host layer the three vocoder modules share (tacotron2_amd/vocoder.py), without a GPU: the packed-row map against a
restatement in numpy, the keys of the packed weight image and of the row-plan cache, the precision / dtype switches and the
argument checks at the head of ``infer``, for WaveGlow, HiFi-GAN and Vocos alike."""
import numpy as np
import pytest
import torch

import hifigan_ref as hr
import vocos_ref as vr
from tacotron2_amd import engine, hifigan, vocoder, vocos, waveglow

CPU = torch.device('cpu')
LABELS = {'waveglow': 'WaveGlow', 'hifigan': 'HiFi-GAN', 'vocos': 'Vocos'}
LENGTHS = ([1], [3, 1], [1, 7, 40])


def _make(kind):
    if kind == 'waveglow':
        return waveglow.WaveGlow(80, 4, 8, 2, 2, dict(n_layers=2, n_channels=64, kernel_size=3))
    if kind == 'hifigan':
        c = hr.CONFIGS['small1']
        return hifigan.Generator(**dict(c, n_mel_channels=80,
                                        resblock_dilation_sizes=[tuple(d) for d in c['resblock_dilation_sizes']]))
    return vocos.Vocos(**vr.CONFIGS['small'])


def _restated(rows, halo, slots=None):
    """The map in numpy: halo marked rows, then per utterance its real rows and slots[b] - rows[b] + halo marked ones."""
    slots = rows if slots is None else slots
    marks = [np.r_[np.full(r, b), np.full(s - r + halo, -1)] for b, (r, s) in enumerate(zip(rows, slots))]
    count = [np.r_[np.arange(r), np.zeros(s - r + halo, int)] for r, s in zip(rows, slots)]
    offs = [halo + sum(s + halo for s in slots[:b]) for b in range(len(rows))]
    return np.r_[np.full(halo, -1), np.r_[tuple(marks)]], np.r_[np.zeros(halo, int), np.r_[tuple(count)]], offs


def _same_map(got, rows, halo, slots=None):
    rowb, rowr, offs, P = got
    wb, wr, wo = _restated(list(rows), halo, None if slots is None else list(slots))
    assert rowb.dtype == torch.int32 and rowr.dtype == torch.int32 and rowb.device == CPU
    assert np.array_equal(rowb.numpy(), wb) and np.array_equal(rowr.numpy(), wr)
    assert offs == wo and P == len(wb) == halo + sum(slots or rows) + halo * len(rows)


# ---------------------------------------------------------------------------------------------------------------
# packed_rows
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", [1, 3, 128])
@pytest.mark.parametrize("lens", LENGTHS)
def test_packed_rows_against_the_restatement(lens, halo):
    _same_map(vocoder.packed_rows(lens, halo), lens, halo)
    _same_map(vocoder.packed_rows(torch.tensor(lens), halo, slots=None), lens, halo)


@pytest.mark.parametrize("halo", [1, 3, 128])
def test_packed_rows_with_slots_wider_than_the_rows(halo):
    rows, slots = [40, 64, 3], [32 * f for f in (2, 2, 1)]
    rowb, rowr, offs, P = got = vocoder.packed_rows(rows, halo, slots)
    _same_map(got, rows, halo, slots)
    assert (rowb >= 0).sum() == 107 and P == halo + sum(slots) + 3 * halo
    assert (rowb[offs[0] + 40:offs[1]] == -1).all() and offs[1] - offs[0] == 64 + halo      # the partial frame, then the halo


@pytest.mark.parametrize("lens", LENGTHS)
def test_the_four_class_methods_are_the_same_map(lens):
    wg, hg, vc = _make('waveglow'), _make('hifigan'), _make('vocos')
    spf = waveglow.HOP // wg.n_group
    _same_map(wg.packed_plan(lens), [spf * n for n in lens], wg.halo())
    rows = [spf * n - (5 if n > 1 else 29) for n in lens]                      # a partial last frame in every utterance
    _same_map(wg.forward_plan(rows, lens), rows, wg.halo(), [spf * n for n in lens])
    _same_map(wg.forward_plan([40, 64, 3], [2, 2, 1]), [40, 64, 3], wg.halo(), [64, 64, 32])
    _same_map(hg.packed_plan(lens), lens, hg.halo_frames())
    rowb0, rowr0, utt, offs, P = vc.packed_plan(lens)
    _same_map((rowb0, rowr0, offs, P), lens, vocos.HALO)
    assert utt.dtype == torch.int32 and utt.tolist() == [[o, n] for o, n in zip(offs, lens)]


# ---------------------------------------------------------------------------------------------------------------
# the packed weight image: one key for the three modules
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(LABELS))
def test_pack_cache_sees_every_kind_of_weight_update(kind):
    m = _make(kind)
    pk = m._packed(CPU)
    assert m._packed(CPU) is pk

    def repacked():
        nonlocal pk
        new = m._packed(CPU)
        fresh, pk = new is not pk, new
        return fresh and m._packed(CPU) is new

    with torch.no_grad():
        next(m.parameters()).mul_(0.5)                                         # in place: torch's version counter
    assert repacked()
    list(m.parameters())[-1].data.mul_(0.5)                                    # through .data: no counter sees it ...
    assert m._packed(CPU) is pk
    engine.bump_weight_generation()                                            # ... the engine's weight generation does
    assert repacked()
    m.load_state_dict(m.state_dict())
    assert repacked()
    m.to(torch.float32)                                                        # any _apply
    assert m._pack is None and repacked()
    if kind == 'vocos':
        m.head.istft.window.mul_(0.5)                                          # a buffer the image is built from
        assert repacked()


# ---------------------------------------------------------------------------------------------------------------
# the row-plan cache
# ---------------------------------------------------------------------------------------------------------------
def _plan(m, kind, lens, dev, forward=False):
    """(the cached plan, the host map it must hold)."""
    if kind != 'waveglow':
        return m._plan(lens, dev), m.packed_plan(lens)
    spf = waveglow.HOP // m.n_group
    if forward:
        rows = [spf * n - 3 for n in lens]
        return m._plan(dev, rows, lens), m.forward_plan(rows, lens)
    return m._plan(dev, lens), m.packed_plan(lens)


@pytest.mark.parametrize("kind", sorted(LABELS))
def test_plan_cache_is_keyed_by_all_the_map_depends_on(kind):
    m = _make(kind)

    def right(plan, want, dev):
        assert plan[0].device.type == dev.type and torch.equal(plan[0], want[0]) and torch.equal(plan[1], want[1])
        assert plan[-1] == want[-1]                                            # P
        if kind == 'vocos':
            assert torch.equal(plan[2], want[2])
        if kind == 'waveglow':
            assert plan[2] == want[2]                                          # offsets

    a, want = _plan(m, kind, [1, 7, 40], CPU)
    right(a, want, CPU)
    again = _plan(m, kind, [1, 7, 40], CPU)[0]
    assert again is a and all(x is y for x, y in zip(again, a))                # the same tensors
    b, want = _plan(m, kind, [40, 40, 40], CPU)                                # other lengths
    assert b is not a
    right(b, want, CPU)
    c, want = _plan(m, kind, [1, 7, 40], CPU)                                  # one entry: the first plan was dropped
    assert c is not a
    right(c, want, CPU)
    cpu0 = torch.device('cpu', 0)                                              # another device string
    d, want = _plan(m, kind, [1, 7, 40], cpu0)
    assert d is not c and str(cpu0) != str(CPU)
    right(d, want, cpu0)
    if kind == 'waveglow':
        e, want = _plan(m, kind, [1, 7, 40], cpu0, forward=True)               # the other direction, the same lengths
        assert e is not d
        right(e, want, cpu0)
        f, want = _plan(m, kind, [1, 7, 40], cpu0)
        assert f is not e
        right(f, want, cpu0)
    assert m._plan_cache is not None
    m.to(torch.float32)
    assert m._plan_cache is None


# ---------------------------------------------------------------------------------------------------------------
# precision / dtype and the head of infer
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(LABELS))
def test_precision_and_dtype_switches(kind):
    m, label = _make(kind), LABELS[kind]
    mod = {'waveglow': waveglow, 'hifigan': hifigan, 'vocos': vocos}[kind]
    assert mod.PRECISIONS is vocoder.PRECISIONS == {'fp32': 0, 'bf16x3': 1, 'bf16': 2}
    assert m.LABEL == label and m.precision == 'fp32' and m.half_io is False
    with pytest.raises(ValueError, match=r"^%s: precision must be one of \['bf16', 'bf16x3', 'fp32'\], got 'fp16'" % label):
        m.precision = 'fp16'
    with pytest.raises(ValueError, match="^%s: precision must be" % label):
        type(m)(**dict(_config(m), precision='tf32'))
    bad = dict(_config(m), precision='tf32', n_mel_channels=0 if kind != 'waveglow' else 81)
    with pytest.raises(ValueError, match="n_mel_channels"):                    # the geometry is judged first
        type(m)(**bad)
    assert m.precision == 'fp32'
    m.precision = 'bf16x3'
    assert m.half() is m and m.precision == 'bf16' and m.half_io is True
    assert all(p.dtype == torch.float32 for p in m.parameters()) and all(b.dtype == torch.float32 for b in m.buffers())
    out = torch.zeros(2, 3)
    assert m._io(out).dtype == torch.float16
    assert m.float() is m and m.precision == 'fp32' and m.half_io is False
    assert m._io(out) is out


def _config(m):
    if isinstance(m, waveglow.WaveGlow):
        return dict(n_mel_channels=80, n_flows=4, n_group=8, n_early_every=2, n_early_size=2,
                    WN_config=dict(n_layers=2, n_channels=64, kernel_size=3))
    return m.config()


@pytest.mark.parametrize("kind", sorted(LABELS))
def test_check_mels_refuses_with_the_class_label(kind):
    m, label = _make(kind), LABELS[kind]
    nm = m.n_mel_channels
    mel = torch.zeros(3, nm, 40)
    assert m._check_mels(mel, None, "infer") == (3, nm, 40, [40, 40, 40])
    assert m._check_mels(mel.half(), torch.tensor([1, 7, 40]), "infer") == (3, nm, 40, [1, 7, 40])
    assert m._check_mels(mel.bfloat16(), (40, 1, 2), "nll") == (3, nm, 40, [40, 1, 2])

    def refused(match, mel, lengths=None, who="infer"):
        with pytest.raises(ValueError, match=match) as e:
            m._check_mels(mel, lengths, who)
        assert str(e.value).startswith("%s.%s: " % (label, who))

    refused(r"expected \(B, %d, N\) mels, got \(%d, 40\)" % (nm, nm), mel[0])                         # rank
    refused(r"expected \(B, %d, N\) mels, got \(3, 40, %d\)" % (nm, nm), mel.transpose(1, 2), who="nll")     # channels
    refused("expected .* got <class 'list'>", [[0.0]])                                            # not a tensor
    refused("mels must be float32, float16 or bfloat16, got torch.int32", mel.int())
    refused("mels must be float32", mel.double())
    refused(r"lengths \[40, 40\] do not fit 3 utterances of 40 frames", mel, [40, 40])
    refused(r"lengths \[40, 0, 40\] do not fit", mel, [40, 0, 40])
    refused(r"lengths \[40, 41, 40\] do not fit", mel, torch.tensor([40, 41, 40]))
    refused(r"lengths \[\] do not fit 0 utterances", mel[:0])                                     # B = 0
    refused("do not fit 3 utterances of 0 frames", mel[:, :, :0])


def test_checkpoint_source_opens_a_wrapper_but_not_a_tensor_entry():
    inner, t = {'a.weight': torch.zeros(2)}, torch.zeros(3)
    mod = torch.nn.Linear(2, 2)
    assert vocoder.checkpoint_source({'model': inner, 'iteration': 3}, 'model') is inner
    assert vocoder.checkpoint_source({'generator': mod}, 'generator') is mod
    assert vocoder.checkpoint_source(inner, 'model') is inner and vocoder.checkpoint_source(mod, 'model') is mod
    flat = {'model': t, 'a.weight': t}                                         # a state dict with an entry of that name
    assert vocoder.checkpoint_source(flat, 'model') is flat
    for load in (waveglow.load_waveglow, hifigan.load_hifigan, vocos.load_vocos):
        with pytest.raises(TypeError, match="^%s: expected a path, a state dict or a module, got int" % load.__name__):
            load(3)
