"""The Vocos fine-tuning driver without a GPU: configuration merging and ``--set``, the refusals, a whole run in validate-only
mode (every host check of generate, MelLoss, their backward and FusedAdam; no kernel runs), and the checkpoint round trip
through ``load_vocos`` and ``checkpoint_path``."""
import json
import os

import pytest
import torch

from tacotron2_amd import native
from tacotron2_amd import vocos_train as vt
from tacotron2_amd.vocos import load_vocos

TINY = ["vocos_config.dim=32", "intermediate_dim=64", "num_layers=1", "training_files=synthetic:5", "batch_size=2",
        "segment_length=2048", "epochs=1", "iters_per_checkpoint=1", "learning_rate=0.001"]


def test_config_merging_and_set(tmp_path):
    cfg = vt.load_config()
    assert cfg == vt.DEFAULTS and cfg is not vt.DEFAULTS
    assert set(cfg) == {'train_config', 'data_config', 'dist_config', 'vocos_config'}
    for key in ('precision', 'learning_rate', 'batch_size', 'seed', 'epochs', 'iters_per_checkpoint', 'checkpoint_path'):
        assert key in cfg['train_config']
    assert 'segment_length' in cfg['data_config']
    path = tmp_path / "config.json"
    path.write_text(json.dumps({'train_config': {'epochs': 3}, 'vocos_config': {'dim': 64}}))
    cfg = vt.load_config(str(path), ["batch_size=4", "train_config.precision=bf16x3", "padding=center", "mel_fmax=null"])
    assert cfg['train_config']['epochs'] == 3 and cfg['vocos_config']['dim'] == 64 and cfg['train_config']['batch_size'] == 4
    assert cfg['train_config']['precision'] == 'bf16x3' and cfg['vocos_config']['padding'] == 'center'
    assert cfg['data_config']['mel_fmax'] is None and cfg['vocos_config']['num_layers'] == 8
    assert vt.DEFAULTS['train_config']['batch_size'] == 16
    with pytest.raises(KeyError, match="ambiguous"):
        vt.load_config(None, ["hop_length=128"])                      # in data_config and in vocos_config
    with pytest.raises(KeyError, match="does not exist"):
        vt.load_config(None, ["sigma=1.0"])
    with pytest.raises(ValueError, match="key=value"):
        vt.load_config(None, ["epochs"])
    path.write_text(json.dumps({'train_config': {'sigma': 1.0}}))
    with pytest.raises(KeyError, match="unknown configuration key train_config.sigma"):
        vt.load_config(str(path))


def test_shared_load_config_with_toy_defaults(tmp_path):
    """``vocoder_train.load_config`` alone: the defaults and the name in the messages are the caller's."""
    from tacotron2_amd import vocoder_train as vtr
    toy = {'a': dict(x=1, y='s', flag=False), 'b': dict(x=2.5, z=3, deep=dict(w=0))}
    cfg = vtr.load_config(toy, "toy_train")
    assert cfg == toy and cfg is not toy and cfg['b']['deep'] is not toy['b']['deep']
    cfg = vtr.load_config(toy, "toy_train", None, ["a.x=7", "b.deep.w=0.25", "y=null", "flag=true", "z=-4", "w=text"])
    assert cfg == {'a': dict(x=7, y=None, flag=True), 'b': dict(x=2.5, z=-4, deep=dict(w='text'))}
    assert type(cfg['a']['x']) is int and cfg['a']['flag'] is True
    assert vtr.load_config(toy, "toy_train", None, ["b.deep.w=0.25"])['b']['deep']['w'] == 0.25
    assert toy['a'] == dict(x=1, y='s', flag=False) and toy['b']['deep'] == dict(w=0)
    with pytest.raises(KeyError, match=r"toy_train: configuration key x is ambiguous: \[\('a', 'x'\), \('b', 'x'\)\]"):
        vtr.load_config(toy, "toy_train", None, ["x=1"])
    with pytest.raises(KeyError, match="toy_train: configuration key a.z does not exist"):
        vtr.load_config(toy, "toy_train", None, ["a.z=1"])
    with pytest.raises(ValueError, match="toy_train: --set takes key=value, got 'z'"):
        vtr.load_config(toy, "toy_train", None, ["z"])
    path = tmp_path / "toy.json"
    path.write_text(json.dumps({'b': {'z': 9, 'deep': {'w': 1}}}))
    assert vtr.load_config(toy, "toy_train", str(path), ["z=10"])['b'] == dict(x=2.5, z=10, deep=dict(w=1))
    path.write_text(json.dumps({'b': {'deep': {'v': 1}}}))
    with pytest.raises(KeyError, match="toy_train: unknown configuration key b.deep.v"):
        vtr.load_config(toy, "toy_train", str(path))
    with pytest.raises(KeyError, match="other_train: unknown configuration key b.deep.v"):
        vtr.load_config(toy, "other_train", str(path))


def test_refusals():
    for bad, match in ((["precision=fp16"], "precision"), (["n_mel_channels=40"], "80 mel channels"),
                       (["segment_length=16000"], "multiple of the hop"), (["vocos_config.hop_length=128"], "not the data's"),
                       (["segment_length=256"], "at least two hops")):
        with pytest.raises(ValueError, match=match):
            vt.check_config(vt.load_config(None, bad))
    assert vt.check_config(vt.load_config()) == (64, 64)
    if not torch.cuda.is_available():
        with pytest.raises(native.NativeError, match="no MI355X"):
            vt.train(1, 0, '', vt.load_config(None, TINY))


def test_run_and_checkpoint_round_trip_validate_only(native_lib, tmp_path, capsys):
    out = str(tmp_path / "out")
    native.set_validate_only(True)
    try:
        it, last = vt.main(["--set", "output_directory=" + out] + [a for s in TINY for a in ("--set", s)])
        assert it == 1 and isinstance(last, float)                     # 5 recordings, batches of 2: iterations 0 and 1
        lines = capsys.readouterr().out.splitlines()
        assert [l.split(':')[0] for l in lines if l[:1].isdigit()] == ['0', '1']
        assert sorted(os.listdir(out)) == ['vocos_0', 'vocos_1']
        ckpt = torch.load(os.path.join(out, 'vocos_1'), map_location='cpu', weights_only=False)
        assert set(ckpt) == {'state_dict', 'iteration', 'optimizer', 'learning_rate', 'vocos_config'}
        assert ckpt['iteration'] == 1 and ckpt['vocos_config']['dim'] == 32 and ckpt['learning_rate'] == 0.001
        voc = load_vocos(os.path.join(out, 'vocos_1'))
        assert voc.config() == ckpt['vocos_config']
        for k, v in voc.state_dict().items():
            assert torch.equal(v, ckpt['state_dict'][k]), k
        # continue from it: the geometry is the checkpoint's, the iteration the one after the saved one
        out2 = str(tmp_path / "out2")
        it, _ = vt.main(["--set", "output_directory=" + out2, "--set", "checkpoint_path=" + os.path.join(out, 'vocos_1'),
                         "--set", "epochs=2"] + [a for s in TINY[3:8:2] + TINY[4:6] for a in ("--set", s)])
        assert it == 3 and sorted(os.listdir(out2)) == ['vocos_2', 'vocos_3']
        resumed = torch.load(os.path.join(out2, 'vocos_2'), map_location='cpu', weights_only=False)
        assert resumed['vocos_config'] == ckpt['vocos_config']
        assert resumed['optimizer']['state'][0]['step'] == 3.0          # FusedAdam's moments came along: two steps, then one
    finally:
        native.set_validate_only(False)
