"""The Vocos fine-tuning driver end to end on the MI355X, as test_zz14 drives WaveGlow's: a child process trains seven
iterations and writes two checkpoints, a second child continues from the first checkpoint and must print the same bits.

The geometry is the smallest the row kernels accept (8 frames per segment, D = 32, I = 64, one layer): what
tests/test_vocos_train_cpu.py runs in validate-only mode, where no kernel runs.  That the loss falls is NOT asserted: seven
steps on changing batches of a one-layer model do not promise it."""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["vocos_config.dim=32", "intermediate_dim=64", "num_layers=1", "training_files=synthetic:8", "batch_size=2",
        "segment_length=2048", "iters_per_checkpoint=3", "max_iterations=6", "learning_rate=0.001"]
KEYS = {'state_dict', 'iteration', 'optimizer', 'learning_rate', 'vocos_config'}


def _drive(out, extra, seconds=240):
    cmd = [sys.executable, "-m", "tacotron2_amd.vocos_train"]
    for item in TINY + ["output_directory=" + out] + extra:
        cmd += ["--set", item]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=seconds)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = {}
    for line in r.stdout.splitlines():
        head, _, val = line.partition(":\t")
        if head.isdigit() and val:
            lines[int(head)] = val
    return lines


def test_driver_trains_checkpoints_and_resumes_with_the_same_bits(native_lib, tmp_path):
    from tacotron2_amd.vocos import load_vocos
    out = str(tmp_path / "run")
    first = _drive(out, [])
    print("driver: " + "  ".join("%d: %s" % kv for kv in sorted(first.items())))
    assert sorted(first) == list(range(7)), sorted(first)
    assert all(math.isfinite(float(v)) for v in first.values()), first
    assert sorted(os.listdir(out)) == ['vocos_0', 'vocos_3', 'vocos_6']
    ckpts = {n: torch.load(os.path.join(out, "vocos_%d" % n), map_location='cpu', weights_only=False) for n in (3, 6)}
    for n, ckpt in ckpts.items():
        assert set(ckpt) == KEYS and ckpt['iteration'] == n and ckpt['learning_rate'] == 0.001, (n, sorted(ckpt))
        assert ckpt['vocos_config']['dim'] == 32 and ckpt['vocos_config']['intermediate_dim'] == 64
        assert ckpt['optimizer']['state'][0]['step'] == n + 1
    assert any(not torch.equal(v, ckpts[6]['state_dict'][k]) for k, v in ckpts[3]['state_dict'].items())

    again = _drive(str(tmp_path / "resumed"), ["checkpoint_path=" + os.path.join(out, "vocos_3")])
    assert sorted(again) == [4, 5, 6], sorted(again)
    assert {k: first[k] for k in again} == again, (first, again)
    resumed = torch.load(os.path.join(str(tmp_path / "resumed"), "vocos_6"), map_location='cpu', weights_only=False)
    for k, v in ckpts[6]['state_dict'].items():
        assert torch.equal(resumed['state_dict'][k], v), k

    voc = load_vocos(os.path.join(out, "vocos_6"))
    assert voc.config() == ckpts[6]['vocos_config']
    sd = voc.state_dict()
    assert set(sd) == set(ckpts[6]['state_dict'])
    for k, v in sd.items():
        assert torch.equal(v, ckpts[6]['state_dict'][k]) and torch.isfinite(v).all(), k
