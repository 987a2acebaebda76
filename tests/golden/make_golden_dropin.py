"""Golden fixtures of tests/test_reference_dropin_cpu.py: what the UNMODIFIED reference computes on the cases that test
holds this repository to, recorded so that the test needs nothing outside the repository.

    python tests/golden/make_golden_dropin.py        # writes tests/golden/live_<seed>.pt, dropin_collate.pt

Runs only where the reference tree lies (make_golden.REF).
  * live_<seed>.pt: the reference's model.py / loss_function.py on four more training cases, through make_golden's shim
    and its assertions (state_dict bit-identical under the seed; outputs, loss, all 60 gradients and the BatchNorm buffers
    equal to the oracle's).  Beside make_golden's digest, every gradient too large to be stored whole is kept at every
    GRAD_STRIDE-th element (``grad_strided``).
  * dropin_collate.pt: the reference's data_utils.py ``TextMelCollate`` on 60 random ragged batches (ties in text length,
    1-item batches, n_frames_per_step 1..4): dtype, shape and SHA-256 of the bytes of every tensor of each 5-tuple.
"""
import hashlib
import importlib.util
import os
import sys
import types

import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the repository root and tests/ on sys.path)
import golden_util as gu  # noqa: E402

GRAD_STRIDE = 16

# (seed, in_lens, out_lens, extra hparams): the parametrisation of test_oracle_equals_reference_live_on_more_cases
LIVE_CASES = [
    (101, [9, 9, 3], [14, 6, 21], ""),                       # tie in text length, longest mel not first
    (202, [15, 2], [3, 17], ",mask_padding=False"),
    (303, [6], [9], ",p_attention_dropout=0.3,p_decoder_dropout=0.2,gate_threshold=0.4"),
    # a smaller attention geometry (hparams.py:65-70): the engine runs it zero-embedded, tests/test_zz1 holds it to this oracle
    (404, [11, 8, 3], [9, 16, 5], ",attention_dim=96,attention_location_n_filters=16,attention_location_kernel_size=17"),
]


def tensor_digest(t):
    return str(t.dtype), tuple(t.shape), hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def make_live(ref_model, ref_loss):
    for seed, in_lens, out_lens, extra in LIVE_CASES:
        case = dict(kind="train", hp=gu.TINY_HP + extra, seed=seed, in_lens=in_lens, out_lens=out_lens)
        name = "live_%d" % seed
        fx, grads = mg.run_train_case(name, case, ref_model, ref_loss)
        fx["grad_stride"] = GRAD_STRIDE
        fx["grad_strided"] = {k: v.reshape(-1)[::GRAD_STRIDE].clone() for k, v in grads.items() if v.numel() > 4096}
        torch.save(fx, os.path.join(gu.GOLDEN_DIR, name + ".pt"))


def make_collate():
    for name in ("librosa", "unidecode", "inflect", "librosa.filters", "librosa.util"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["librosa.filters"].mel = lambda *a, **k: None
    for attr in ("pad_center", "tiny", "normalize"):
        setattr(sys.modules["librosa.util"], attr, None)
    sys.path.insert(0, mg.REF)
    spec = importlib.util.spec_from_file_location("reference_data_utils", os.path.join(mg.REF, "data_utils.py"))
    ref_data = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_data)
    sys.path.remove(mg.REF)
    from tacotron2_amd.data_utils import TextMelCollate
    digests = []
    for r, items in gu.collate_items(torch.Generator().manual_seed(2024)):
        want = ref_data.TextMelCollate(r)(items)
        for a, b in zip(want, TextMelCollate(r)(items)):
            assert a.dtype == b.dtype and torch.equal(a, b), r
        digests.append([tensor_digest(t) for t in want])
    torch.save({"seed": 2024, "digests": digests}, os.path.join(gu.GOLDEN_DIR, "dropin_collate.pt"))


def main():
    torch.set_num_threads(8)
    real_dropout = torch.nn.functional.dropout
    try:
        make_live(*mg.import_reference())
    finally:
        torch.nn.functional.dropout = real_dropout
    make_collate()


if __name__ == "__main__":
    main()
