"""Fine-tuning driver for the Vocos vocoder on the MI355X with a mel-reconstruction loss, shaped like ``waveglow_train``:

    python -m tacotron2_amd.vocos_train -c config.json [-r rank -g group_name]
    python -m tacotron2_amd.vocos_train --set training_files=synthetic:240 --set output_directory=out --set epochs=2
    python -m tacotron2_amd.multiproc -m tacotron2_amd.vocos_train -c config.json           # one rank per GPU

One step is ``Mel2Samp`` segments -> ``batch_mels`` -> ``vc.generate(mel)`` -> ``MelLoss`` -> ``backward()`` -> ``FusedAdam``:
the masked mean |log-mel(generated) - log-mel(recording)|, the dominant term of Vocos's and HiFi-GAN's objectives and, alone,
the usual recipe for fine-tuning a vocoder on a Tacotron's predicted mels.  There is no discriminator here.  With
``stft_loss_weight`` = lambda > 0 the step's loss is ``MelLoss + lambda MultiResolutionSTFTLoss(generated, recording segment)``
(``stft_resolutions``: a list of [filter_length, hop_length, win_length], null for the module's default); with ``padding='center'``
the generated audio is shorter than the segment and the recording's first samples are compared.  With the weight 0 the second
loss is not even constructed.

Frames.  A segment of ``segment_length`` = hop N samples has N + 1 mel frames; the model is given the first N.  With
``padding='same'``, ``generate`` returns hop N samples, whose mel again has N + 1 frames: the loss compares frames [0, N).
With ``padding='center'`` the model returns hop (N - 1) samples with N frames, all compared.  ``segment_length`` must be a
multiple of the hop.

The configuration has the sections ``train_config`` (output_directory, epochs, learning_rate, iters_per_checkpoint, batch_size,
seed, checkpoint_path, precision, with_tensorboard, max_iterations, stft_loss_weight, stft_resolutions), ``data_config`` (the arguments of ``Mel2Samp``),
``dist_config`` and ``vocos_config`` (the Vocos geometry; with ``checkpoint_path`` the geometry is the checkpoint's and
``hop_length`` / ``padding`` are taken from here).  ``--set key=value`` overrides a key (dotted path, or a bare key that occurs
in exactly one section).  ``precision`` is the model's (fp32, bf16x3 or bf16); the loss's backward runs in split-bf16 unless
the model is fp32.  A checkpoint ``vocos_{iteration}`` holds ``{'state_dict', 'iteration', 'optimizer', 'learning_rate',
'vocos_config'}``; ``load_vocos`` reads it back, and ``checkpoint_path`` continues from it with the batches the interrupted run
would have seen.  One line per iteration, ``"{iteration}:\\t{loss:.9f}"``; the loss is read back after the whole step has been
enqueued, and ``MelLoss`` runs without a range check of the generated samples (it would cost a host synchronisation).
There is no CPU compute path: without an MI355X the driver raises.
"""
import torch

from . import vocoder_train as vtr
from .audio import MelLoss, MultiResolutionSTFTLoss
from .vocoder import PRECISIONS
from .vocos import Vocos, load_vocos

WHO = 'vocos_train'
DEFAULTS = {
    'train_config': dict(precision='fp32', output_directory='checkpoints', epochs=100000, learning_rate=2e-4,
                         iters_per_checkpoint=2000, batch_size=16, seed=1234, checkpoint_path='', with_tensorboard=False,
                         max_iterations=None, stft_loss_weight=0.0, stft_resolutions=None),
    'data_config': dict(training_files='train_files.txt', segment_length=16384, sampling_rate=22050, filter_length=1024,
                        hop_length=256, win_length=1024, mel_fmin=0.0, mel_fmax=8000.0),
    'dist_config': dict(dist_backend='nccl', dist_url='tcp://localhost:54321'),
    'vocos_config': dict(n_mel_channels=80, dim=512, intermediate_dim=1536, num_layers=8, n_fft=1024, hop_length=256,
                         padding='same'),
}


def load_config(path=None, overrides=()):
    """The defaults, then the JSON file (any subset of the sections), then the ``key=value`` overrides."""
    return vtr.load_config(DEFAULTS, WHO, path, overrides)


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
    weight = t['stft_loss_weight']
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not weight >= 0:
        raise ValueError("vocos_train: stft_loss_weight must be a number >= 0, got %r" % (weight,))
    if weight > 0:
        res = MultiResolutionSTFTLoss.DEFAULT_RESOLUTIONS if t['stft_resolutions'] is None else t['stft_resolutions']
        generated = S - hop if v['padding'] == 'center' else S
        for L, _, _ in MultiResolutionSTFTLoss.check_resolutions(res):
            if L // 2 >= generated:
                raise ValueError("vocos_train: the STFT loss resolution with filter_length %d reflect-pads by %d, the generated "
                                 "audio has %d samples" % (L, L // 2, generated))
    return N, N


def make_model(config):
    t, v = config['train_config'], config['vocos_config']
    if t['checkpoint_path']:
        model = load_vocos(t['checkpoint_path'], precision=t['precision'], hop_length=v['hop_length'], padding=v['padding'])
        config['vocos_config'] = model.config()
    else:
        model = Vocos(precision=t['precision'], **v)
    return model


def _payload(model, optimizer, learning_rate, iteration, vocos_config):
    return dict(state_dict=vtr.cpu_state(model), iteration=iteration, optimizer=optimizer.state_dict(),
                learning_rate=learning_rate, vocos_config=vocos_config)


def save_checkpoint(model, optimizer, learning_rate, iteration, vocos_config, filepath):
    vtr.save_checkpoint(_payload(model, optimizer, learning_rate, iteration, vocos_config), filepath)


def resume(checkpoint_path, optimizer):
    """FusedAdam's moments and the iteration of a checkpoint of this driver (a bare state dict has neither) -> iteration."""
    ckpt = torch.load(checkpoint_path, map_location='cpu', weights_only=False)
    if not (isinstance(ckpt, dict) and 'vocos_config' in ckpt):
        return -1
    if 'optimizer' in ckpt:
        optimizer.load_state_dict(ckpt['optimizer'])
    print("Loaded checkpoint '{}' (iteration {})".format(checkpoint_path, ckpt.get('iteration', 0)))
    return int(ckpt.get('iteration', 0))


def train_step(model, loss_fn, optimizer, mel, n_in, n_cmp, loss_precision, stft_loss=None, stft_weight=0.0, recording=None):
    """One step on (B, 80, >= n_in) target log-mels -> the loss (a 0-d device tensor with its graph already consumed).  With
    ``stft_loss`` (a ``MultiResolutionSTFTLoss``) the loss is ``loss_fn + stft_weight stft_loss(generated, recording)``."""
    model.zero_grad()
    audio = model.generate(mel[:, :, :n_in].contiguous())
    loss = loss_fn(audio, mel[:, :, :n_cmp], precision=loss_precision)
    if stft_loss is not None:
        loss = loss + stft_weight * stft_loss(audio, recording, precision=loss_precision)
    loss.backward()
    optimizer.step()
    return loss.detach()


def train(num_gpus, rank, group_name, config):
    t = config['train_config']
    n_in, n_cmp = check_config(config)
    loss_precision = 'fp32' if t['precision'] == 'fp32' else 'bf16x3'

    def make_step(model, optimizer, trainset, num_gpus):
        loss_fn = MelLoss(trainset_stft(trainset))
        # the geometry is the model's (a checkpoint's wins): 'center' returns hop (N - 1) samples, N frames, all compared
        compared = n_in if config['vocos_config']['padding'] == 'center' else n_cmp
        weight = float(t['stft_loss_weight'])
        stft_loss = MultiResolutionSTFTLoss(t['stft_resolutions']) if weight > 0 else None
        return lambda audio, mel: vtr.shown_loss(                 # all-reduced AFTER the optimizer's step
            train_step(model, loss_fn, optimizer, mel, n_in, compared, loss_precision, stft_loss, weight, audio), num_gpus)

    return vtr.train(
        WHO, num_gpus, rank, group_name, config, make_step=make_step, make_model=lambda: make_model(config),
        resume=lambda model, optimizer: resume(t['checkpoint_path'], optimizer),
        checkpoint=lambda *state: (_payload(*state, config['vocos_config']), "vocos_{}"))


def trainset_stft(trainset):
    """The data set's own front end (built on first use by ``batch_mels``): the loss measures with the table that made the
    targets."""
    from .audio import TacotronSTFT
    if trainset._stft is None:
        trainset._stft = TacotronSTFT(*trainset.stft_args)
    return trainset._stft


def main(argv=None):
    return vtr.main(WHO, __doc__, DEFAULTS, train, argv)


if __name__ == '__main__':
    main()
