"""This repository against what the UNMODIFIED reference computes, on cases beyond tests/test_oracle_golden.py's: the
reference's results were recorded by tests/golden/make_golden_dropin.py (which asserts the same equalities against the
live reference before it writes anything) as tests/golden/live_<seed>.pt and tests/golden/dropin_collate.pt, so that
nothing outside the repository is read here.
"""
import hashlib

import pytest
import torch

import golden_util as gu
from oracle import tacotron2_oracle as orc


def _close(a, b, tol, what):
    """make_golden.close: max |a - b| within tol x max(1, max |b|)."""
    err = (a.double() - b.double()).abs().max().item()
    ref = b.double().abs().max().item()
    assert err <= tol * max(1.0, ref), "%s: max abs err %.3e (ref max %.3e)" % (what, err, ref)


def test_collate_equals_reference_on_random_ragged_batches():
    """TextMelCollate against the reference's on 60 random ragged batches (ties in text length, 1-item batches,
    n_frames_per_step 1..4): every tensor of the 5-tuple bit-identical, dtypes included (dtype, shape and SHA-256 of the
    bytes of the reference's tensors)."""
    from tacotron2_amd.data_utils import TextMelCollate
    fx = gu.load_fixture("dropin_collate")
    cases = gu.collate_items(torch.Generator().manual_seed(fx["seed"]))
    assert len(cases) == len(fx["digests"]) == 60
    for case, ((r, items), want) in enumerate(zip(cases, fx["digests"])):
        got = TextMelCollate(r)(items)
        assert len(got) == len(want) == 5
        for t, (dtype, shape, sha) in zip(got, want):
            assert str(t.dtype) == dtype and tuple(t.shape) == shape, (case, r)
            assert hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest() == sha, (case, r)


@pytest.mark.parametrize("seed,in_lens,out_lens,extra", [
    (101, [9, 9, 3], [14, 6, 21], ""),                       # tie in text length, longest mel not first
    (202, [15, 2], [3, 17], ",mask_padding=False"),
    (303, [6], [9], ",p_attention_dropout=0.3,p_decoder_dropout=0.2,gate_threshold=0.4"),
    # a smaller attention geometry (hparams.py:65-70): the engine runs it zero-embedded, tests/test_zz1 holds it to this oracle
    (404, [11, 8, 3], [9, 16, 5], ",attention_dim=96,attention_location_n_filters=16,attention_location_kernel_size=17"),
])
def test_oracle_equals_reference_live_on_more_cases(seed, in_lens, out_lens, extra):
    """The oracle's pin, widened beyond tests/test_oracle_golden.py's fixtures: the reference's model.py on further shapes
    and hyper-parameters, with the reference's dropout masks.  The weights regenerated from the seed are the ones the
    reference initialised; outputs, loss, all 60 gradients (whole when small, else norm + every 16th element) and the
    BatchNorm buffers equal to the reference's at make_golden's tolerances."""
    fx = gu.load_fixture("live_%d" % seed)
    assert (fx["hp"], fx["seed"], fx["in_lens"], fx["out_lens"]) == (gu.TINY_HP + extra, seed, in_lens, out_lens)
    hp = gu.make_hparams(fx["hp"])
    sd = gu.build_state_dict(hp, seed)
    assert set(sd) >= set(fx["sd_digest"])
    for k, d in fx["sd_digest"].items():
        f = sd[k].double().reshape(-1)
        assert abs(f.sum().item() - d["sum"]) <= 1e-6 * max(1.0, d["abssum"]), k
        assert torch.equal(f[d["idx"]].float(), d["sample"]), "weights regenerated from the seed differ: %s" % k
    batch = gu.make_train_batch(in_lens, out_lens, hp.n_mel_channels, seed)
    loss, out, grads, bufs = orc.train_step_grads(sd, hp, batch, gu.unpack_masks(fx["masks"]))
    for i, nm in enumerate(("mel", "mel_post", "gate", "align")):
        _close(out[i], fx["outputs"][i], 2e-5, nm)
    _close(loss, fx["loss"], 1e-6, "loss")
    assert set(grads) == set(fx["grad_digest"]) and len(grads) == 60
    stride = fx["grad_stride"]
    for k, d in fx["grad_digest"].items():
        g = grads[k].double().reshape(-1)
        assert abs(g.norm().item() - d["l2"]) <= 1e-4 * d["l2"] + 2e-6, k
        if k in fx["grad_small"]:
            _close(grads[k], fx["grad_small"][k], 5e-5, "grad " + k)
        else:
            _close(g[::stride], fx["grad_strided"][k], 5e-5, "grad " + k)
    assert set(fx["grad_small"]) | set(fx["grad_strided"]) == set(grads)
    for k, v in fx["buffers"].items():
        _close(bufs[k].float(), v.float(), 1e-6, "buffer " + k)
