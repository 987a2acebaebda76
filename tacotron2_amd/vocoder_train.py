"""What the vocoder training drivers (``waveglow_train``, ``vocos_train``) share: everything that does not depend on the model.

``load_config`` merges a driver's defaults, a JSON file and the ``--set key=value`` overrides; ``train`` is the body of a
driver's ``train()`` from the device gate to the last iteration, given the driver's model, first iteration, step and
checkpoint payload; ``main`` is the command line both answer to (``-c -r -g --n_gpus --set``).  ``who`` is the driver's name,
the prefix of every message.

The order of the batches and the start of every segment are functions of (seed, epoch, position): ``epoch_batches`` and the
slice of the first resumed epoch in ``train`` are what makes a run continued from ``checkpoint_path`` see the batches the
interrupted run would have seen.  The loss a step returns is read back once per iteration, after the whole step has been
enqueued; where in its step a driver all-reduces that loss (``shown_loss``) is the driver's own business, so the sequence of
collectives per rank is the step's.
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


def _merge(dst, src, where, who):
    for k, v in src.items():
        if k not in dst:
            raise KeyError("%s: unknown configuration key %s%s" % (who, where, k))
        if isinstance(dst[k], dict):
            _merge(dst[k], v, where + k + '.', who)
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


def load_config(defaults, who, path=None, overrides=()):
    """A copy of ``defaults``, then the JSON file (any subset of the sections), then the ``key=value`` overrides (dotted
    path, or a bare key that occurs in exactly one section)."""
    cfg = copy.deepcopy(defaults)
    if path:
        with open(path) as fh:
            _merge(cfg, json.load(fh), '', who)
    for item in overrides:
        if '=' not in item:
            raise ValueError("%s: --set takes key=value, got %r" % (who, item))
        key, text = item.split('=', 1)
        want = tuple(key.split('.'))
        hits = [p for p in _paths(cfg) if p == want or (len(want) == 1 and p[-1] == want[0])]
        if len(hits) != 1:
            raise KeyError("%s: configuration key %s %s" % (who, key, "is ambiguous: %s" % hits if hits else "does not exist"))
        node = cfg
        for k in hits[0][:-1]:
            node = node[k]
        node[hits[0][-1]] = _value(text)
    return cfg


def init_distributed(rank, num_gpus, group_name, dist_backend, dist_url):
    """NVIDIA's ``init_distributed``: one process per GPU.  RANK / WORLD_SIZE in the environment (torch.distributed.run)
    win over the flags."""
    if 'RANK' in os.environ and 'WORLD_SIZE' in os.environ:
        rank, num_gpus = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
        dist_url = 'env://'
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    if not torch.cuda.is_available():
        raise native.NativeError("vocoder_train: distributed mode requires an MI355X")
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', rank)) % torch.cuda.device_count())
    if not dist.is_initialized():
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        dist.init_process_group(dist_backend, init_method=dist_url, world_size=num_gpus, rank=rank)
    return rank, num_gpus


def epoch_batches(n_items, batch_size, seed, epoch, rank=0, num_gpus=1):
    """The index lists of this rank's batches of one epoch: a permutation seeded by (seed, epoch), dealt to the ranks in
    turn (``DistributedSampler``'s rule), the incomplete last batch dropped."""
    perm = torch.randperm(n_items, generator=torch.Generator().manual_seed(int(seed) + int(epoch))).tolist()
    mine = perm[rank:n_items - n_items % num_gpus:num_gpus]
    return [mine[i:i + batch_size] for i in range(0, len(mine) - batch_size + 1, batch_size)]


def shown_loss(loss, num_gpus):
    """The loss to print: its mean over the ranks (a collective, so a step calls this at its own fixed place), or itself."""
    return reduce_tensor(loss, num_gpus) if num_gpus > 1 else loss.detach()


def cpu_state(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


def save_checkpoint(payload, filepath):
    print("Saving model and optimizer state at iteration {} to {}".format(payload['iteration'], filepath))
    tmp = filepath + '.tmp'
    torch.save(payload, tmp)
    os.replace(tmp, filepath)


def train(who, num_gpus, rank, group_name, config, make_model, resume, make_step, checkpoint):
    """-> (last iteration, its loss).  The driver supplies, and ``train`` calls in this order:
      ``make_model()`` -> the module, before it is moved to the device and made data-parallel;
      ``resume(model, optimizer)`` -> the iteration of the checkpoint at ``checkpoint_path`` (only when that is set), having
        loaded it into both;
      ``make_step(model, optimizer, trainset, num_gpus)`` -> ``step(audio, mel)``, which runs one whole iteration on a collated
        batch and its mels and returns the 0-d tensor to print (see ``shown_loss``);
      ``checkpoint(model, optimizer, learning_rate, iteration)`` -> (the payload to save, the file stem, ``"waveglow_{}"``)."""
    t = config['train_config']
    if not torch.cuda.is_available() and not native.validate_only():
        raise native.NativeError("%s: no MI355X visible and the engine has no CPU path" % who)
    if num_gpus > 1:
        rank, num_gpus = init_distributed(rank, num_gpus, group_name, **config['dist_config'])
    torch.manual_seed(t['seed'])
    if torch.cuda.is_available():
        torch.cuda.manual_seed(t['seed'])

    model = make_model()
    if torch.cuda.is_available():
        model = model.cuda()
    if num_gpus > 1:
        model = apply_gradient_allreduce(model)
    learning_rate = float(t['learning_rate'])
    optimizer = FusedAdam(model.parameters(), lr=learning_rate)
    iteration = 0
    if t['checkpoint_path']:
        iteration = resume(model, optimizer) + 1                  # the iteration after the saved one

    trainset = Mel2Samp(seed=t['seed'], **config['data_config'])
    step = make_step(model, optimizer, trainset, num_gpus)
    per_epoch = len(epoch_batches(len(trainset), t['batch_size'], t['seed'], 0, rank, num_gpus))
    if per_epoch == 0:
        raise ValueError("%s: %d recordings are less than one batch of %d on %d rank(s)"
                         % (who, len(trainset), t['batch_size'], num_gpus))
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
            last = float(step(audio, trainset.batch_mels(audio)).item())
            print("{}:\t{:.9f}".format(iteration, last), flush=True)
            if logger is not None:
                logger.add_scalar('training_loss', last, iteration)
            if iteration % t['iters_per_checkpoint'] == 0 and rank == 0:
                payload, stem = checkpoint(model, optimizer, learning_rate, iteration)
                save_checkpoint(payload, os.path.join(t['output_directory'], stem.format(iteration)))
            iteration += 1
            if t['max_iterations'] is not None and iteration > t['max_iterations']:
                return iteration - 1, last
    return iteration - 1, last


def main(who, doc, defaults, train, argv=None, config_help='JSON file with the configuration sections'):
    """The command line of a driver: ``train`` is its ``train(num_gpus, rank, group_name, config)``."""
    ap = argparse.ArgumentParser(description=doc.split('\n')[0])
    ap.add_argument('-c', '--config', type=str, default=None, help=config_help)
    ap.add_argument('-r', '--rank', type=int, default=0, help='rank of this process')
    ap.add_argument('-g', '--group_name', type=str, default='', help='name of the group of processes')
    ap.add_argument('--n_gpus', type=int, default=None, help='number of ranks (default: WORLD_SIZE, else 1)')
    ap.add_argument('--set', action='append', default=[], metavar='key=value', help='override a configuration key')
    args = ap.parse_args(argv)
    config = load_config(defaults, who, args.config, args.set)
    num_gpus = args.n_gpus if args.n_gpus is not None else int(os.environ.get('WORLD_SIZE', 1))
    return train(num_gpus, args.rank, args.group_name, config)
