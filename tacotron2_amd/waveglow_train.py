"""Training driver for WaveGlow on the MI355X, with the surface of NVIDIA's WaveGlow ``train.py``:

    python -m tacotron2_amd.waveglow_train -c config.json [-r rank -g group_name]
    python -m tacotron2_amd.waveglow_train --set training_files=synthetic:240 --set output_directory=out --set epochs=2
    python -m tacotron2_amd.multiproc -m tacotron2_amd.waveglow_train -c config.json        # one rank per GPU

The configuration has NVIDIA's sections and defaults: ``train_config`` (output_directory, epochs, learning_rate, sigma,
iters_per_checkpoint, batch_size, seed, checkpoint_path, with_tensorboard, fp16_run), ``data_config`` (the arguments of
``Mel2Samp``), ``dist_config`` and ``waveglow_config``; ``--set key=value`` overrides a key (dotted path, or a bare key
that occurs in exactly one section), so that no file is needed.  The model is trained in glow.py's own parametrisation
(``weight_g`` / ``weight_v``, ``WaveGlow(weight_norm=True)``) by ``optim.FusedAdam``; one line per iteration,
``"{iteration}:\\t{loss:.9f}"``.

What is different from NVIDIA's driver:
  * ``fp16_run=True`` selects ``precision='bf16'`` (bf16 products, f32 master weights, no loss scaling); ``precision`` may
    also be given directly: fp32, bf16x3 or bf16;
  * a checkpoint ``waveglow_{iteration}`` holds ``{'model': state_dict, 'iteration', 'optimizer', 'learning_rate',
    'waveglow_config'}``: the state dict (NVIDIA's training keys) rather than the pickled module, which needs glow.py
    importable to be read.  ``load_waveglow`` reads it, and ``model.load_state_dict(ckpt['model'])`` loads it into glow.py's
    training module;
  * the order of the batches and the start of every segment are functions of (seed, epoch, position), so a run resumed
    from ``checkpoint_path`` continues with the batches the interrupted run would have seen;
  * the loss is read back once per iteration, after the whole step has been enqueued.
There is no CPU compute path: without an MI355X the driver raises.
"""
import os

import torch

from . import vocoder_train as vtr
from .vocoder_train import epoch_batches, init_distributed  # noqa: F401  (this driver's surface)
from .waveglow import PRECISIONS, WaveGlow

WHO = 'waveglow_train'
DEFAULTS = {
    'train_config': dict(fp16_run=False, precision=None, output_directory='checkpoints', epochs=100000, learning_rate=1e-4,
                         sigma=1.0, iters_per_checkpoint=2000, batch_size=12, seed=1234, checkpoint_path='',
                         with_tensorboard=False, max_iterations=None),
    'data_config': dict(training_files='train_files.txt', segment_length=16000, sampling_rate=22050, filter_length=1024,
                        hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0),
    'dist_config': dict(dist_backend='nccl', dist_url='tcp://localhost:54321'),
    'waveglow_config': dict(n_mel_channels=80, n_flows=12, n_group=8, n_early_every=4, n_early_size=2,
                            WN_config=dict(n_layers=8, n_channels=256, kernel_size=3)),
}


def load_config(path=None, overrides=()):
    """NVIDIA's defaults, then the JSON file (any subset of the sections), then the ``key=value`` overrides."""
    return vtr.load_config(DEFAULTS, WHO, path, overrides)


def precision_of(train_config):
    p = train_config.get('precision')
    if p is None:
        return 'bf16' if train_config.get('fp16_run') else 'fp32'
    if p not in PRECISIONS:
        raise ValueError("waveglow_train: precision must be one of %s, got %r" % (sorted(PRECISIONS), p))
    return p


def _payload(model, optimizer, learning_rate, iteration, waveglow_config):
    return dict(model=vtr.cpu_state(model), iteration=iteration, optimizer=optimizer.state_dict(),
                learning_rate=learning_rate, waveglow_config=waveglow_config)


def save_checkpoint(model, optimizer, learning_rate, iteration, waveglow_config, filepath):
    vtr.save_checkpoint(_payload(model, optimizer, learning_rate, iteration, waveglow_config), filepath)


def load_checkpoint(checkpoint_path, model, optimizer):
    """-> (model, optimizer, iteration): weights (g / v), FusedAdam's moments (from a checkpoint of this driver) and the
    iteration of the checkpoint."""
    assert os.path.isfile(checkpoint_path), "no checkpoint at '%s'" % checkpoint_path
    ckpt = torch.load(checkpoint_path, map_location='cpu', weights_only=False)
    sd = ckpt['model'].state_dict() if isinstance(ckpt['model'], torch.nn.Module) else ckpt['model']
    if not any(k.endswith('.weight_g') for k in sd):             # a folded checkpoint: v = w, g = ||w||
        sd = WaveGlow.from_state_dict(sd, weight_norm=True).state_dict()
    model.load_state_dict(sd)
    if 'optimizer' in ckpt and 'waveglow_config' in ckpt:        # an optimizer state is indexed by parameter ORDER: ours only
        optimizer.load_state_dict(ckpt['optimizer'])
    print("Loaded checkpoint '{}' (iteration {})".format(checkpoint_path, ckpt.get('iteration', 0)))
    return model, optimizer, int(ckpt.get('iteration', 0))


def train(num_gpus, rank, group_name, config):
    t, waveglow_config = config['train_config'], config['waveglow_config']
    sigma = float(t['sigma'])

    def make_step(model, optimizer, trainset, num_gpus):
        def step(audio, mel):
            model.zero_grad()
            loss = model.training_loss(mel, audio.to(mel.device), sigma)
            shown = vtr.shown_loss(loss, num_gpus)                # all-reduced BEFORE the backward's gradient exchange
            loss.backward()
            optimizer.step()
            return shown
        return step

    return vtr.train(
        WHO, num_gpus, rank, group_name, config, make_step=make_step,
        make_model=lambda: WaveGlow(precision=precision_of(t), weight_norm=True, **waveglow_config),
        resume=lambda model, optimizer: load_checkpoint(t['checkpoint_path'], model, optimizer)[2],
        checkpoint=lambda *state: (_payload(*state, waveglow_config), "waveglow_{}"))


def main(argv=None):
    return vtr.main(WHO, __doc__, DEFAULTS, train, argv, config_help="JSON file with NVIDIA's configuration sections")


if __name__ == '__main__':
    main()
