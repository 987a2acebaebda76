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
import argparse
import copy
import json
import os

import torch
import torch.distributed as dist

from . import native
from .distributed import apply_gradient_allreduce, reduce_tensor
from .mel2samp import Mel2Samp
from .optim import FusedAdam
from .waveglow import PRECISIONS, WaveGlow

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


def _merge(dst, src, where):
    for k, v in src.items():
        if k not in dst:
            raise KeyError("waveglow_train: unknown configuration key %s%s" % (where, k))
        if isinstance(dst[k], dict):
            _merge(dst[k], v, where + k + '.')
        else:
            dst[k] = v


def _paths(cfg, prefix=()):
    for k, v in cfg.items():
        if isinstance(v, dict):
            yield from _paths(v, prefix + (k,))
        else:
            yield prefix + (k,)


def _value(text):
    try:
        return json.loads(text)
    except ValueError:
        return {'true': True, 'false': False, 'none': None}.get(text.lower(), text)


def load_config(path=None, overrides=()):
    """NVIDIA's defaults, then the JSON file (any subset of the sections), then the ``key=value`` overrides."""
    cfg = copy.deepcopy(DEFAULTS)
    if path:
        with open(path) as fh:
            _merge(cfg, json.load(fh), '')
    for item in overrides:
        if '=' not in item:
            raise ValueError("waveglow_train: --set takes key=value, got %r" % item)
        key, text = item.split('=', 1)
        want = tuple(key.split('.'))
        hits = [p for p in _paths(cfg) if p == want or (len(want) == 1 and p[-1] == want[0])]
        if len(hits) != 1:
            raise KeyError("waveglow_train: configuration key %s %s" % (key, "is ambiguous: %s" % hits if hits else "does not exist"))
        node = cfg
        for k in hits[0][:-1]:
            node = node[k]
        node[hits[0][-1]] = _value(text)
    return cfg


def precision_of(train_config):
    p = train_config.get('precision')
    if p is None:
        return 'bf16' if train_config.get('fp16_run') else 'fp32'
    if p not in PRECISIONS:
        raise ValueError("waveglow_train: precision must be one of %s, got %r" % (sorted(PRECISIONS), p))
    return p


def init_distributed(rank, num_gpus, group_name, dist_backend, dist_url):
    """NVIDIA's ``init_distributed``: one process per GPU.  RANK / WORLD_SIZE in the environment (torch.distributed.run)
    win over the flags."""
    if 'RANK' in os.environ and 'WORLD_SIZE' in os.environ:
        rank, num_gpus = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
        dist_url = 'env://'
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    if not torch.cuda.is_available():
        raise native.NativeError("waveglow_train: distributed mode requires an MI355X")
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', rank)) % torch.cuda.device_count())
    if not dist.is_initialized():
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        dist.init_process_group(dist_backend, init_method=dist_url, world_size=num_gpus, rank=rank)
    return rank, num_gpus


def save_checkpoint(model, optimizer, learning_rate, iteration, waveglow_config, filepath):
    print("Saving model and optimizer state at iteration {} to {}".format(iteration, filepath))
    payload = dict(model={k: v.detach().cpu() for k, v in model.state_dict().items()}, iteration=iteration,
                   optimizer=optimizer.state_dict(), learning_rate=learning_rate, waveglow_config=waveglow_config)
    tmp = filepath + '.tmp'
    torch.save(payload, tmp)
    os.replace(tmp, filepath)


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


def epoch_batches(n_items, batch_size, seed, epoch, rank=0, num_gpus=1):
    """The index lists of this rank's batches of one epoch: a permutation seeded by (seed, epoch), dealt to the ranks in
    turn (``DistributedSampler``'s rule), the incomplete last batch dropped."""
    perm = torch.randperm(n_items, generator=torch.Generator().manual_seed(int(seed) + int(epoch))).tolist()
    mine = perm[rank:n_items - n_items % num_gpus:num_gpus]
    return [mine[i:i + batch_size] for i in range(0, len(mine) - batch_size + 1, batch_size)]


def train(num_gpus, rank, group_name, config):
    t, data_config, dist_config, waveglow_config = (config[k] for k in ('train_config', 'data_config', 'dist_config',
                                                                         'waveglow_config'))
    if not torch.cuda.is_available() and not native.validate_only():
        raise native.NativeError("waveglow_train: no MI355X visible and the engine has no CPU path")
    if num_gpus > 1:
        rank, num_gpus = init_distributed(rank, num_gpus, group_name, **dist_config)
    torch.manual_seed(t['seed'])
    if torch.cuda.is_available():
        torch.cuda.manual_seed(t['seed'])

    model = WaveGlow(precision=precision_of(t), weight_norm=True, **waveglow_config)
    if torch.cuda.is_available():
        model = model.cuda()
    if num_gpus > 1:
        model = apply_gradient_allreduce(model)
    learning_rate, sigma = float(t['learning_rate']), float(t['sigma'])
    optimizer = FusedAdam(model.parameters(), lr=learning_rate)
    iteration = 0
    if t['checkpoint_path']:
        model, optimizer, iteration = load_checkpoint(t['checkpoint_path'], model, optimizer)
        iteration += 1                                            # the iteration after the saved one

    trainset = Mel2Samp(seed=t['seed'], **data_config)
    per_epoch = len(epoch_batches(len(trainset), t['batch_size'], t['seed'], 0, rank, num_gpus))
    if per_epoch == 0:
        raise ValueError("waveglow_train: %d recordings are less than one batch of %d on %d rank(s)"
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
            model.zero_grad()
            audio = trainset.collate([trainset[i] for i in idx])
            mel = trainset.batch_mels(audio)
            loss = model.training_loss(mel, audio.to(mel.device), sigma)
            shown = reduce_tensor(loss, num_gpus) if num_gpus > 1 else loss.detach()
            loss.backward()
            optimizer.step()
            last = float(shown.item())
            print("{}:\t{:.9f}".format(iteration, last), flush=True)
            if logger is not None:
                logger.add_scalar('training_loss', last, iteration)
            if iteration % t['iters_per_checkpoint'] == 0 and rank == 0:
                save_checkpoint(model, optimizer, learning_rate, iteration, waveglow_config,
                                os.path.join(t['output_directory'], "waveglow_{}".format(iteration)))
            iteration += 1
            if t['max_iterations'] is not None and iteration > t['max_iterations']:
                return iteration - 1, last
    return iteration - 1, last


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('-c', '--config', type=str, default=None, help='JSON file with NVIDIA\'s configuration sections')
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
