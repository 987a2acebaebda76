"""Fine-tuning driver for the Vocos vocoder on the MI355X with a mel-reconstruction loss, shaped like ``waveglow_train``:

    python -m tacotron2_amd.vocos_train -c config.json [-r rank -g group_name]
    python -m tacotron2_amd.vocos_train --set training_files=synthetic:240 --set output_directory=out --set epochs=2
    python -m tacotron2_amd.multiproc -m tacotron2_amd.vocos_train -c config.json           # one rank per GPU

One step is ``Mel2Samp`` segments -> ``batch_mels`` -> ``vc.generate(mel)`` -> ``MelLoss`` -> ``backward()`` -> ``FusedAdam``:
the masked mean |log-mel(generated) - log-mel(recording)|, the dominant term of Vocos's and HiFi-GAN's objectives and, alone,
the usual recipe for fine-tuning a vocoder on a Tacotron's predicted mels.  There is no discriminator here.

Frames.  A segment of ``segment_length`` = hop N samples has N + 1 mel frames; the model is given the first N.  With
``padding='same'``, ``generate`` returns hop N samples, whose mel again has N + 1 frames: the loss compares frames [0, N).
With ``padding='center'`` the model returns hop (N - 1) samples with N frames, all compared.  ``segment_length`` must be a
multiple of the hop.

The configuration has the sections ``train_config`` (output_directory, epochs, learning_rate, iters_per_checkpoint, batch_size,
seed, checkpoint_path, precision, with_tensorboard, max_iterations), ``data_config`` (the arguments of ``Mel2Samp``),
``dist_config`` and ``vocos_config`` (the Vocos geometry; with ``checkpoint_path`` the geometry is the checkpoint's and
``hop_length`` / ``padding`` are taken from here).  ``--set key=value`` overrides a key (dotted path, or a bare key that occurs
in exactly one section).  ``precision`` is the model's (fp32, bf16x3 or bf16); the loss's backward runs in split-bf16 unless
the model is fp32.  A checkpoint ``vocos_{iteration}`` holds ``{'state_dict', 'iteration', 'optimizer', 'learning_rate',
'vocos_config'}``; ``load_vocos`` reads it back, and ``checkpoint_path`` continues from it with the batches the interrupted run
would have seen.  One line per iteration, ``"{iteration}:\\t{loss:.9f}"``; the loss is read back after the whole step has been
enqueued, and ``MelLoss`` runs without a range check of the generated samples (it would cost a host synchronisation).
There is no CPU compute path: without an MI355X the driver raises.
"""
import argparse
import copy
import json
import os

import torch

from . import native
from .audio import MelLoss
from .distributed import apply_gradient_allreduce, reduce_tensor
from .mel2samp import Mel2Samp
from .optim import FusedAdam
from .vocoder import PRECISIONS
from .vocos import Vocos, load_vocos
from .waveglow_train import _paths, _value, epoch_batches, init_distributed

DEFAULTS = {
    'train_config': dict(precision='fp32', output_directory='checkpoints', epochs=100000, learning_rate=2e-4,
                         iters_per_checkpoint=2000, batch_size=16, seed=1234, checkpoint_path='', with_tensorboard=False,
                         max_iterations=None),
    'data_config': dict(training_files='train_files.txt', segment_length=16384, sampling_rate=22050, filter_length=1024,
                        hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0),
    'dist_config': dict(dist_backend='nccl', dist_url='tcp://localhost:54321'),
    'vocos_config': dict(n_mel_channels=80, dim=512, intermediate_dim=1536, num_layers=8, n_fft=1024, hop_length=256,
                         padding='same'),
}


def _merge(dst, src, where):
    for k, v in src.items():
        if k not in dst:
            raise KeyError("vocos_train: unknown configuration key %s%s" % (where, k))
        if isinstance(dst[k], dict):
            _merge(dst[k], v, where + k + '.')
        else:
            dst[k] = v


def load_config(path=None, overrides=()):
    """The defaults, then the JSON file (any subset of the sections), then the ``key=value`` overrides."""
    cfg = copy.deepcopy(DEFAULTS)
    if path:
        with open(path) as fh:
            _merge(cfg, json.load(fh), '')
    for item in overrides:
        if '=' not in item:
            raise ValueError("vocos_train: --set takes key=value, got %r" % item)
        key, text = item.split('=', 1)
        want = tuple(key.split('.'))
        hits = [p for p in _paths(cfg) if p == want or (len(want) == 1 and p[-1] == want[0])]
        if len(hits) != 1:
            raise KeyError("vocos_train: configuration key %s %s" % (key, "is ambiguous: %s" % hits if hits else "does not exist"))
        node = cfg
        for k in hits[0][:-1]:
            node = node[k]
        node[hits[0][-1]] = _value(text)
    return cfg


def check_config(config):
    """Refuse what the step cannot run: -> (frames given to the model, frames the loss compares)."""
    t, d, v = config['train_config'], config['data_config'], config['vocos_config']
    if t['precision'] not in PRECISIONS:
        raise ValueError("vocos_train: precision must be one of %s, got %r" % (sorted(PRECISIONS), t['precision']))
    if v['n_mel_channels'] != 80:
        raise ValueError("vocos_train: Mel2Samp computes 80 mel channels, the model takes %d" % v['n_mel_channels'])
    if v['hop_length'] != d['hop_length'] or v['n_fft'] != d['filter_length']:
        raise ValueError("vocos_train: the model's n_fft %d / hop %d are not the data's filter_length %d / hop_length %d"
                         % (v['n_fft'], v['hop_length'], d['filter_length'], d['hop_length']))
    hop, S = d['hop_length'], d['segment_length']
    if S % hop or S < 2 * hop or S <= d['filter_length'] // 2:
        raise ValueError("vocos_train: segment_length %d must be a multiple of the hop %d, at least two hops and more than "
                         "half a frame" % (S, hop))
    N = S // hop
    return N, N


def make_model(config):
    t, v = config['train_config'], config['vocos_config']
    if t['checkpoint_path']:
        model = load_vocos(t['checkpoint_path'], precision=t['precision'], hop_length=v['hop_length'], padding=v['padding'])
        config['vocos_config'] = model.config()
    else:
        model = Vocos(precision=t['precision'], **v)
    return model


def save_checkpoint(model, optimizer, learning_rate, iteration, vocos_config, filepath):
    print("Saving model and optimizer state at iteration {} to {}".format(iteration, filepath))
    payload = dict(state_dict={k: v.detach().cpu() for k, v in model.state_dict().items()}, iteration=iteration,
                   optimizer=optimizer.state_dict(), learning_rate=learning_rate, vocos_config=vocos_config)
    tmp = filepath + '.tmp'
    torch.save(payload, tmp)
    os.replace(tmp, filepath)


def resume(checkpoint_path, optimizer):
    """FusedAdam's moments and the iteration of a checkpoint of this driver (a bare state dict has neither) -> iteration."""
    ckpt = torch.load(checkpoint_path, map_location='cpu', weights_only=False)
    if not (isinstance(ckpt, dict) and 'vocos_config' in ckpt):
        return -1
    if 'optimizer' in ckpt:
        optimizer.load_state_dict(ckpt['optimizer'])
    print("Loaded checkpoint '{}' (iteration {})".format(checkpoint_path, ckpt.get('iteration', 0)))
    return int(ckpt.get('iteration', 0))


def train_step(model, loss_fn, optimizer, mel, n_in, n_cmp, loss_precision):
    """One step on (B, 80, >= n_in) target log-mels -> the loss (a 0-d device tensor with its graph already consumed)."""
    model.zero_grad()
    audio = model.generate(mel[:, :, :n_in].contiguous())
    loss = loss_fn(audio, mel[:, :, :n_cmp], precision=loss_precision)
    loss.backward()
    optimizer.step()
    return loss.detach()


def train(num_gpus, rank, group_name, config):
    t, data_config, dist_config = config['train_config'], config['data_config'], config['dist_config']
    n_in, n_cmp = check_config(config)
    if not torch.cuda.is_available() and not native.validate_only():
        raise native.NativeError("vocos_train: no MI355X visible and the engine has no CPU path")
    if num_gpus > 1:
        rank, num_gpus = init_distributed(rank, num_gpus, group_name, **dist_config)
    torch.manual_seed(t['seed'])
    if torch.cuda.is_available():
        torch.cuda.manual_seed(t['seed'])

    model = make_model(config)
    vocos_config = config['vocos_config']
    if vocos_config['padding'] == 'center':
        n_cmp = n_in                                              # hop (N - 1) samples: N frames, all compared
    if torch.cuda.is_available():
        model = model.cuda()
    if num_gpus > 1:
        model = apply_gradient_allreduce(model)
    learning_rate = float(t['learning_rate'])
    optimizer = FusedAdam(model.parameters(), lr=learning_rate)
    iteration = 0
    if t['checkpoint_path']:
        iteration = resume(t['checkpoint_path'], optimizer) + 1       # the iteration after the saved one

    trainset = Mel2Samp(seed=t['seed'], **data_config)
    loss_fn = MelLoss(trainset_stft(trainset))
    loss_precision = 'fp32' if t['precision'] == 'fp32' else 'bf16x3'
    per_epoch = len(epoch_batches(len(trainset), t['batch_size'], t['seed'], 0, rank, num_gpus))
    if per_epoch == 0:
        raise ValueError("vocos_train: %d recordings are less than one batch of %d on %d rank(s)"
                         % (len(trainset), t['batch_size'], num_gpus))
    if rank == 0 and not os.path.isdir(t['output_directory']):
        os.makedirs(t['output_directory'])
        os.chmod(t['output_directory'], 0o775)
    logger = None
    if t['with_tensorboard'] and rank == 0:
        from torch.utils.tensorboard import SummaryWriter
        logger = SummaryWriter(os.path.join(t['output_directory'], 'logs'))

    model.train()
    last = None
    for epoch in range(iteration // per_epoch, t['epochs']):
        print("Epoch: {}".format(epoch))
        trainset.set_epoch(epoch)
        batches = epoch_batches(len(trainset), t['batch_size'], t['seed'], epoch, rank, num_gpus)
        for idx in batches[iteration % per_epoch if epoch == iteration // per_epoch else 0:]:
            audio = trainset.collate([trainset[i] for i in idx])
            mel = trainset.batch_mels(audio)
            loss = train_step(model, loss_fn, optimizer, mel, n_in, n_cmp, loss_precision)
            shown = reduce_tensor(loss, num_gpus) if num_gpus > 1 else loss
            last = float(shown.item())
            print("{}:\t{:.9f}".format(iteration, last), flush=True)
            if logger is not None:
                logger.add_scalar('training_loss', last, iteration)
            if iteration % t['iters_per_checkpoint'] == 0 and rank == 0:
                save_checkpoint(model, optimizer, learning_rate, iteration, vocos_config,
                                os.path.join(t['output_directory'], "vocos_{}".format(iteration)))
            iteration += 1
            if t['max_iterations'] is not None and iteration > t['max_iterations']:
                return iteration - 1, last
    return iteration - 1, last


def trainset_stft(trainset):
    """The data set's own front end (built on first use by ``batch_mels``): the loss measures with the table that made the
    targets."""
    from .audio import TacotronSTFT
    if trainset._stft is None:
        trainset._stft = TacotronSTFT(*trainset.stft_args)
    return trainset._stft


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-c', '--config', type=str, default=None, help='JSON file with the configuration sections')
    ap.add_argument('-r', '--rank', type=int, default=0, help='rank of this process')
    ap.add_argument('-g', '--group_name', type=str, default='', help='name of the group of processes')
    ap.add_argument('--n_gpus', type=int, default=None, help='number of ranks (default: WORLD_SIZE, else 1)')
    ap.add_argument('--set', action='append', default=[], metavar='key=value', help='override a configuration key')
    args = ap.parse_args(argv)
    config = load_config(args.config, args.set)
    num_gpus = args.n_gpus if args.n_gpus is not None else int(os.environ.get('WORLD_SIZE', 1))
    return train(num_gpus, args.rank, args.group_name, config)


if __name__ == '__main__':
    main()
