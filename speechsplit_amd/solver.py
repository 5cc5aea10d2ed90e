"""Host-side mirror of the reference's ``Solver`` (boundary B2; reference solver.py:18-269).

Same constructor (``Solver(vcc_loader, config, hparams)``), same ``config`` attributes, same ``train()`` loop
structure, log line and checkpoint files; the six statements of the step body (solver.py:157-172) are ONE C-ABI
call into the HIP engine (``ss_g3_train_step``).  The demo.pkl validation block (solver.py:206-227) and
the ablation forwards (solver.py:245-251) are ``validate``; tensorboard and the matplotlib plots are out of scope.

Data parallelism is new (the reference is single-device): under ``torchrun`` each rank takes its shard of every
batch and of the resampling draws, gradients are summed with one RCCL all-reduce over the flat arena, and every
rank applies the same Adam update (speechsplit_amd/dist.py).
"""
import datetime
import os
import time

import torch

from . import dist as _dist
from .engine import draw_interp
from .model import Generator_3 as Generator
from .model import Generator_6
from .model import InterpLnr
from .staging import DevicePrefetcher
from .utils import pad_seq_to_2, quantize_f0_numpy


def _option(config, name, env, environ):
    """config.<name>, or -- for the unchanged main.py, whose config has no such attribute -- the environment variable (empty: unset)"""
    return getattr(config, name, None) if hasattr(config, name) else (environ.get(env) or None)


def optim_ext_options(config, environ=None):
    """(weight_decay, weight_decay_which, ema_decay or None, ema_warmup) from config.weight_decay / SS_WEIGHT_DECAY, config.weight_decay_which /
    SS_WEIGHT_DECAY_WHICH ('all' | 'weights'), config.ema_decay / SS_EMA_DECAY and config.ema_warmup / SS_EMA_WARMUP, read the way grad_clip
    is read.  Defaults: no decay, 'all', no average, no warm-up.  Needs no device."""
    environ = os.environ if environ is None else environ
    wd = _option(config, 'weight_decay', 'SS_WEIGHT_DECAY', environ)
    wd = float(wd) if wd is not None else 0.0
    if not (0.0 <= wd < float('inf')):
        raise ValueError('weight_decay must be 0 / None (off) or positive and finite, got {!r}'.format(wd))
    which = _option(config, 'weight_decay_which', 'SS_WEIGHT_DECAY_WHICH', environ) or 'all'
    if which not in ('all', 'weights'):
        raise ValueError("weight_decay_which must be 'all' or 'weights', got {!r}".format(which))
    decay = _option(config, 'ema_decay', 'SS_EMA_DECAY', environ)
    decay = float(decay) if decay is not None else None
    if decay is not None and not (0.0 <= decay < 1.0):
        raise ValueError('ema_decay must lie in [0, 1) (None: no average), got {!r}'.format(decay))
    warm = _option(config, 'ema_warmup', 'SS_EMA_WARMUP', environ)
    if isinstance(warm, str):
        if warm.strip().lower() not in ('0', '1', 'true', 'false', 'yes', 'no', 'on', 'off'):
            raise ValueError('ema_warmup must be a boolean (0 / 1), got {!r}'.format(warm))
        warm = warm.strip().lower() in ('1', 'true', 'yes', 'on')
    return wd, which, decay, bool(warm)


LR_SCHEDULE_KINDS = ('constant', 'cosine', 'linear', 'exponential', 'step')


def lr_schedule_options(config, environ=None):
    """The learning-rate schedule as Engine.set_lr_schedule's keyword arguments, or None (off, the default), from config.lr_schedule /
    SS_LR_SCHEDULE ('constant' | 'cosine' | 'linear' | 'exponential' | 'step'; None, '' or 'off': off), config.lr_warmup / SS_LR_WARMUP,
    lr_warmup_start / SS_LR_WARMUP_START, lr_total / SS_LR_TOTAL, lr_gamma / SS_LR_GAMMA, lr_period / SS_LR_PERIOD and lr_min / SS_LR_MIN,
    read the way optim_ext_options reads its options.  Defaults: no warm-up, from 0.1 of the rate, min 0; for cosine and linear lr_total
    defaults to config.num_iters - lr_warmup.  gamma (exponential, step) and period (step) have no default.  Needs no device."""
    environ = os.environ if environ is None else environ
    kind = _option(config, 'lr_schedule', 'SS_LR_SCHEDULE', environ)
    if kind is None or kind == 'off':
        return None
    if kind not in LR_SCHEDULE_KINDS:
        raise ValueError("lr_schedule must be None / 'off' or one of {}, got {!r}".format(', '.join(map(repr, LR_SCHEDULE_KINDS)), kind))

    def number(name, env, cast, default):
        v = _option(config, name, env, environ)
        return cast(v) if v is not None else default

    warmup = number('lr_warmup', 'SS_LR_WARMUP', int, 0)
    if warmup < 0:
        raise ValueError('lr_warmup must be >= 0, got {!r}'.format(warmup))
    start = number('lr_warmup_start', 'SS_LR_WARMUP_START', float, 0.1)
    if not (0.0 < start <= 1.0):
        raise ValueError('lr_warmup_start must lie in (0, 1], got {!r}'.format(start))
    min_lr = number('lr_min', 'SS_LR_MIN', float, 0.0)
    if not (0.0 <= min_lr < float('inf')):
        raise ValueError('lr_min must be >= 0 and finite, got {!r}'.format(min_lr))
    opts = {'kind': kind, 'warmup': warmup, 'warmup_start': start, 'total': None, 'gamma': None, 'period': None, 'min_lr': min_lr}
    if kind in ('cosine', 'linear'):
        total = number('lr_total', 'SS_LR_TOTAL', int, None)
        if total is None:
            total = int(config.num_iters) - warmup
        if total < 1:
            raise ValueError('lr_total must be >= 1 (default num_iters - lr_warmup), got {!r}'.format(total))
        opts['total'] = total
    if kind in ('exponential', 'step'):
        gamma = number('lr_gamma', 'SS_LR_GAMMA', float, None)
        if gamma is None or not (0.0 < gamma <= 1.0):
            raise ValueError('lr_gamma must lie in (0, 1] for {!r} (it has no default), got {!r}'.format(kind, gamma))
        opts['gamma'] = gamma
    if kind == 'step':
        period = number('lr_period', 'SS_LR_PERIOD', int, None)
        if period is None or period < 1:
            raise ValueError("lr_period must be >= 1 for 'step' (it has no default), got {!r}".format(period))
        opts['period'] = period
    return opts


class Solver(object):
    """Solver for training"""

    def __init__(self, vcc_loader, config, hparams):
        self.vcc_loader = vcc_loader
        self.hparams = hparams
        self.num_iters = config.num_iters
        self.g_lr = config.g_lr
        self.beta1 = config.beta1
        self.beta2 = config.beta2
        self.resume_iters = config.resume_iters
        self.use_tensorboard = getattr(config, 'use_tensorboard', False)
        self.rank, self.local_rank, self.world = _dist.world_info()
        # data-parallel exchange (world > 1): 'native' = the engine's own RCCL communicator and bucket schedule (ss_g3_dp_train_step /
        # ss_g6_dp_train_step), 'torch' = torch.distributed all-reduces around the engine's no-Adam step (Engine.dp_train_step).  The native
        # schedule has never run on more than one GPU (the development boxes have one); the torch path is the fallback until it has.
        self.dp_backend = getattr(config, 'dp_backend', None) or os.environ.get('SS_DP_BACKEND', 'native')
        if self.dp_backend not in ('native', 'torch'):
            raise ValueError("dp_backend must be 'native' or 'torch', got {!r}".format(self.dp_backend))
        self.dp_schedule = getattr(config, 'dp_schedule', None) or os.environ.get('SS_DP_SCHEDULE', 'overlap')
        # clip_grad_norm_(G.parameters(), grad_clip) between backward and optimizer.step(), inside the engine's step (Engine.set_grad_clip):
        # config.grad_clip, or -- for the unchanged main.py, whose config has no such attribute -- SS_GRAD_CLIP.  None / 0: no clipping, no norm,
        # the reference's log line; 'inf': no clipping, but the norm is logged and a step with non-finite gradients is skipped.
        clip = getattr(config, 'grad_clip', None) if hasattr(config, 'grad_clip') else (os.environ.get('SS_GRAD_CLIP') or None)
        self.grad_clip = float(clip) if clip is not None else 0.0
        if not self.grad_clip >= 0.0:
            raise ValueError('grad_clip must be 0 / None (off), positive or inf, got {!r}'.format(clip))
        # gradient accumulation: one optimiser step over accum_steps loader batches (SS_STEP_ACCUMULATE): config.accum_steps, or -- for the
        # unchanged main.py -- SS_ACCUM_STEPS.  1 (default): the train loop's calls exactly as without it.  num_iters, the checkpoints and the
        # optimiser state count optimiser steps.
        accum = getattr(config, 'accum_steps', None) if hasattr(config, 'accum_steps') else (os.environ.get('SS_ACCUM_STEPS') or None)
        self.accum_steps = int(accum) if accum is not None else 1
        if self.accum_steps < 1:
            raise ValueError('accum_steps must be a positive integer, got {!r}'.format(accum))
        # decoupled weight decay (AdamW) and an exponential moving average of the parameters, both inside the engine's optimiser step
        # (Engine.set_weight_decay / set_ema); off by default, and then nothing is called and the checkpoints are the reference's
        self.weight_decay, self.weight_decay_which, self.ema_decay, self.ema_warmup = optim_ext_options(config)
        # learning-rate warm-up and decay inside the engine's optimiser step, keyed on the device's step counter (Engine.set_lr_schedule);
        # off by default, and then nothing is called, the log line and the checkpoints are the reference's.  g_lr stays the base rate.
        self.lr_schedule = lr_schedule_options(config)
        self.use_cuda = torch.cuda.is_available()
        if not self.use_cuda:
            raise RuntimeError('speechsplit_amd.Solver needs a ROCm GPU (the engine has no CPU fallback)')
        dev_id = self.local_rank if self.world > 1 else config.device_id
        self.device = torch.device('cuda:{}'.format(dev_id))
        torch.cuda.set_device(self.device)
        self.log_dir = config.log_dir
        self.sample_dir = config.sample_dir
        self.model_save_dir = config.model_save_dir
        self.log_step = config.log_step
        self.sample_step = config.sample_step
        self.model_save_step = config.model_save_step
        self.build_model()

    GENERATOR = Generator          # SolverF0 below trains Generator_6 with the same shell

    def build_model(self):
        per_rank = self.hparams.batch_size // max(self.world, 1)
        self.G = self.GENERATOR(self.hparams, max_batch=per_rank)
        self.Interp = InterpLnr(self.hparams)
        self.print_network(self.G, 'G')
        self.G.to(self.device)                      # creates the engine, parameters now live in its arena
        self.eng = self.G._eng
        self.eng.set_adam(self.g_lr, self.beta1, self.beta2, 1e-8, 0)      # solver.py:62
        self.step_count = 0
        if self.grad_clip:
            self.eng.set_grad_clip(self.grad_clip)
        if self.weight_decay:
            self.eng.set_weight_decay(self.weight_decay, self.weight_decay_which)
        if self.lr_schedule:
            self.eng.set_lr_schedule(**self.lr_schedule)
        if self.world > 1:
            _dist.init('nccl', self.device)
            import torch.distributed as dist
            dist.broadcast(self.eng.params, src=0)   # identical replicas
        if self.ema_decay is not None:               # the average starts as a copy of the (broadcast) parameters
            self.eng.set_ema(self.ema_decay, self.ema_warmup)
        if self.world > 1:
            self.eng.set_lockstep(True)              # never refuse a step on the status word: check() reports it on every rank at the same iteration
            # the engine's own RCCL communicator: its data-parallel step launches the collectives on the engine's streams and costs
            # nothing over the one-GPU step, where torch.distributed's path measured +0.5 ms
            if self.dp_backend == 'native':
                self.eng.comm_init(self.rank, self.world)

    def print_network(self, model, name):
        num_params = sum(p.numel() for p in model.parameters())
        if self.rank == 0:
            print(model)
            print(name)
            print("The number of parameters: {}".format(num_params))

    # ---- checkpoints in the reference's format: {'model': state_dict, 'optimizer': Adam.state_dict()} (solver.py:198-202)
    def optimizer_state_dict(self):
        mv, vv = self.eng.views(self.eng.adam_m), self.eng.views(self.eng.adam_v)
        state = {i: {'step': torch.tensor(float(self.step_count)), 'exp_avg': mv[n].detach().cpu().clone(),
                     'exp_avg_sq': vv[n].detach().cpu().clone()} for i, n in enumerate(self.G._names)}
        group = {'lr': self.g_lr, 'betas': (self.beta1, self.beta2), 'eps': 1e-8, 'weight_decay': self.weight_decay or 0, 'amsgrad': False,
                 'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
                 'params': list(range(len(self.G._names)))}
        if self.weight_decay:
            group['weight_decay_which'] = self.weight_decay_which
        return {'state': state if self.step_count else {}, 'param_groups': [group]}

    def load_optimizer_state_dict(self, sd):
        group = sd['param_groups'][0]
        self.g_lr = group['lr']
        self.beta1, self.beta2 = group['betas']
        mv, vv = self.eng.views(self.eng.adam_m), self.eng.views(self.eng.adam_v)
        step = 0
        for i, n in enumerate(self.G._names):
            st = sd['state'].get(i)
            if st is None:
                continue
            mv[n].copy_(st['exp_avg'])
            vv[n].copy_(st['exp_avg_sq'])
            step = int(st['step'])
        self.step_count = step
        self.eng.set_adam(self.g_lr, self.beta1, self.beta2, group.get('eps', 1e-8), step)
        # A decay the checkpoint was trained with wins, as its lr and betas do.  A checkpoint WITHOUT one (every checkpoint from before the
        # option existed stores 0) leaves a configured decay in force: that is how decay is switched on for a run that is under way.
        stored = float(group.get('weight_decay') or 0.0)
        if stored:
            which = group.get('weight_decay_which', 'all')
            if self.weight_decay and (self.weight_decay, self.weight_decay_which) != (stored, which) and self.rank == 0:
                print('Note: the checkpoint\'s weight decay {} ({}) replaces the configured {} ({})'.format(
                    stored, which, self.weight_decay, self.weight_decay_which))
            self.weight_decay, self.weight_decay_which = stored, which
            self.eng.set_weight_decay(stored, which)
        elif self.weight_decay and self.rank == 0:
            print('Note: the checkpoint was written without weight decay; the configured {} ({}) applies from here on'.format(
                self.weight_decay, self.weight_decay_which))

    def save_model(self, it):
        G_path = os.path.join(self.model_save_dir, '{}-G.ckpt'.format(it))
        ckpt = {'model': {k: v.detach().cpu() for k, v in self.G.state_dict().items()}, 'optimizer': self.optimizer_state_dict()}
        if self.eng.ema is not None:      # the average under the model's keys (buffers as they are: it loads into a fresh generator), and its update count
            ema = self.eng.ema_views()
            ckpt['model_ema'] = {k: (ema[k] if k in ema else v).detach().cpu().clone() for k, v in ckpt['model'].items()}
            ckpt['ema_updates'] = int(self.eng.ema_stats()[0].item())
        if self.lr_schedule:              # the options; the position is the optimiser state's step count
            ckpt['lr_schedule'] = dict(self.lr_schedule)
        torch.save(ckpt, G_path)

    def restore_model(self, resume_iters):
        print('Loading the trained models from step {}...'.format(resume_iters))
        G_path = os.path.join(self.model_save_dir, '{}-G.ckpt'.format(resume_iters))
        ckpt = torch.load(G_path, map_location=lambda storage, loc: storage, weights_only=False)
        self.G.load_state_dict(ckpt['model'])
        self.load_optimizer_state_dict(ckpt['optimizer'])
        # A schedule the checkpoint was trained with wins, as its weight decay does; the restored step count positions it.  A checkpoint
        # without one leaves a configured schedule in force.
        stored = ckpt.get('lr_schedule')
        if stored:
            if self.lr_schedule and dict(stored) != self.lr_schedule and self.rank == 0:
                print('Note: the checkpoint\'s learning-rate schedule {} replaces the configured {}'.format(dict(stored), self.lr_schedule))
            self.lr_schedule = dict(stored)
            self.eng.set_lr_schedule(**self.lr_schedule)
        elif self.lr_schedule and self.rank == 0:
            print('Note: the checkpoint was written without a learning-rate schedule; the configured {} applies from here on'.format(
                self.lr_schedule))
        if self.ema_decay is not None:
            if 'model_ema' in ckpt:       # the average and its update count back; parameters without an average of their own start one
                flat = self.eng.params.clone()
                views = self.eng.views(flat)
                for k, v in ckpt['model_ema'].items():
                    if k in views:
                        views[k].copy_(v)
                self.eng.set_ema(self.ema_decay, self.ema_warmup, state=(flat, int(ckpt.get('ema_updates', 0))))
            else:
                if self.rank == 0:
                    print('Note: the checkpoint holds no parameter average; the EMA starts from the restored parameters')
                self.eng.set_ema(self.ema_decay, self.ema_warmup)
        elif 'model_ema' in ckpt and self.rank == 0:
            print('Warning: the checkpoint holds a parameter average (\'model_ema\', {} updates) but no ema_decay is configured: it is not '
                  'restored and the next checkpoint will not carry one'.format(ckpt.get('ema_updates', 0)))

    # ---- one iteration of solver.py:141-172 on a collated batch
    N_DRAWS = 4                    # InterpLnr calls per step: the outer one and Encoder_7's three (SolverF0: Encoder_6's three)

    def _shard(self, batch, draws):
        """This rank's part of a collated batch and of its draws (drawn here, as the reference does, when none are given)."""
        x_real_org, emb_org, f0_org, len_org = batch
        per_rank = getattr(self.vcc_loader, 'per_rank', False)       # the loader already produced this rank's shard
        Bg = x_real_org.shape[0] * (self.world if per_rank else 1)
        if draws is None:
            draws = draw_interp(Bg, self.N_DRAWS, self.hparams)      # same generator calls, same order as the reference
        if self.world > 1:
            if not per_rank:
                x_real_org, emb_org, f0_org, len_org = _dist.shard_batch(batch, self.rank, self.world)
            draws = _dist.shard_draws(draws[0], draws[1], Bg, self.rank, self.world)
        return (x_real_org, emb_org, f0_org, len_org), draws

    def _step(self, batch, draws, last=True, accumulate=False, grad_scale=1.0):
        """One engine step on a collated batch.  last: the step that applies the optimiser (data parallel: the one that all-reduces); otherwise
        backward only, on this rank alone.  accumulate: the backward adds to the gradient arena."""
        (x_real_org, emb_org, f0_org, len_org), draws = self._shard(batch, draws)
        to = dict(device=self.device, non_blocking=True)
        # a batch whose frame count is not hparams.max_len_pad is a length bucket (speechsplit_amd/buckets.py): max_len_pad = T
        bucket = x_real_org.shape[1] != self.hparams.max_len_pad
        args = (x_real_org.to(**to), f0_org.to(**to), emb_org.to(**to), len_org.to(**to), draws)
        if not last:
            return self.eng.g3_train_step(*args, no_adam=True, bucket=bucket, accumulate=accumulate)
        if self.world > 1 and self.dp_backend == 'torch':
            return self.eng.dp_train_step(*args, self.world, schedule=self.dp_schedule, bucket=bucket, accumulate=accumulate)
        if self.world > 1:
            return self.eng.dp_train_step_native(*args, bucket=bucket, accumulate=accumulate)
        return self.eng.g3_train_step(*args, grad_scale=grad_scale, bucket=bucket, accumulate=accumulate)

    def train_on_batch(self, batch, draws=None):
        """One optimiser step.  batch: a collated batch, or a LIST of k collated batches (with a list of k draws, or None) -- the
        micro-batches of one accumulation cycle, whose gradients are summed in the engine's arena and applied once with the mean of their
        means; each may be a length bucket of its own.  Returns the loss on the device: of the batch, or the mean of the k losses."""
        if not isinstance(batch[0], (list, tuple)):
            loss = self._step(batch, draws)
            self.step_count += 1
            return loss
        k = len(batch)
        draws = [None] * k if draws is None else draws
        if k < 1 or len(draws) != k:
            raise ValueError('train_on_batch: a list of k batches takes a list of k draws (or None)')
        if k == 1:
            return self.train_on_batch(batch[0], draws[0])
        total = None
        for j in range(k):
            loss = self._step(batch[j], draws[j], last=j == k - 1, accumulate=j > 0, grad_scale=1.0 / k)
            total = loss.clone() if total is None else total.add_(loss)      # the engine's loss word is rewritten by the next call
        self.step_count += 1
        return total.div_(k)

    # ---- validation on demo.pkl-style data (solver.py:206-227) and the ablation forwards of solver.py:245-251 (no plots)
    def validate(self, validation_pt, ablations=False, ema=False):
        """validation_pt: list of [speaker, emb f32[1,82], (mel f32[L,80], f0 f32[L], L, uid)] (assets/demo.pkl layout).
        Returns (mean sum-reduced MSE, per-utterance dict of outputs).  G stays in eval mode afterwards, as in the reference.
        ema: on the averaged weights (inside Engine.ema_weights(); the parameters have their bits back afterwards)."""
        if ema:
            with self.eng.ema_weights():
                return self.validate(validation_pt, ablations)
        import numpy as np
        self.G = self.G.eval()
        losses, outs = [], {}
        with torch.no_grad():
            for val_sub in validation_pt:
                emb = torch.from_numpy(np.asarray(val_sub[1], np.float32)).to(self.device)
                mel, f0, L = val_sub[2][0], val_sub[2][1], val_sub[2][2]
                x_real_pad, _ = pad_seq_to_2(mel[np.newaxis, :, :], 192)                                   # solver.py:213
                f0_pad = np.pad(f0, (0, 192 - L), 'constant', constant_values=(0, 0))                      # :215
                onehot = torch.from_numpy(quantize_f0_numpy(f0_pad)[0][np.newaxis]).to(self.device)        # :216-218
                x_real = torch.from_numpy(x_real_pad.astype(np.float32)).to(self.device)
                x_f0 = torch.cat((x_real, onehot), dim=-1)
                out = self.G(x_f0, x_real, emb)                                                            # :221
                losses.append(float(torch.nn.functional.mse_loss(x_real, out, reduction='sum')))           # :222
                rec = {'out': out}
                if ablations:                                                                              # :245-251
                    rec['woF'] = self.G(torch.cat((x_real, torch.zeros_like(onehot)), -1), x_real, emb)
                    rec['woR'] = self.G(x_f0, torch.zeros_like(x_real), emb)
                    rec['woC'] = self.G(torch.cat((torch.zeros_like(x_real), onehot), -1), x_real, emb)
                outs[val_sub[0]] = rec
        return float(np.mean(losses)), outs

    def train(self):
        data_loader = self.vcc_loader
        data_iter = DevicePrefetcher(data_loader, self.device)       # next batch staged H2D while this step runs
        validation_pt = getattr(self, 'validation_pt', None)
        if validation_pt is None and os.path.exists('assets/demo.pkl'):   # solver.py:16
            import pickle
            validation_pt = pickle.load(open('assets/demo.pkl', 'rb'))
        start_iters = 0
        if self.resume_iters:
            print('Resuming ...')
            start_iters = self.resume_iters
            self.num_iters += self.resume_iters
            self.restore_model(self.resume_iters)
        if self.rank == 0:
            print('Current learning rates, g_lr: {}.'.format(self.g_lr))
            print('Start training...')
        keys = ['G/loss_id']
        start_time = time.time()
        # The log line's loss is read WITHOUT draining the GPU: on a log step the loss is copied to pinned host memory behind the step
        # (non-blocking) and the line is printed once that copy has landed -- an iteration or two later, same text, same order.  A blocking
        # .item() every log_step iterations left the GPU waiting for the host to enqueue the next step again: 0.2 ms per iteration at
        # log_step = 10 (bench.py solver_loop: 5.51 vs 5.29 ms for the bare step).
        pending = []                      # (copy-done event, pinned loss, iteration, elapsed text, pinned clip stats or None, pinned lr stats or None)
        skipped_seen = 0

        def flush(block):
            nonlocal skipped_seen
            while pending and (block or pending[0][0].query()):
                ev, host_loss, it, et, host_clip, host_lr = pending.pop(0)
                ev.synchronize()
                if self.rank == 0:
                    log = "Elapsed [{}], Iteration [{}/{}]".format(et, it, self.num_iters)
                    for tag in keys:
                        log += ", {}: {:.8f}".format(tag, float(host_loss))
                    if host_clip is not None:                     # {norm before clipping, coefficient, steps clipped, steps skipped}
                        log += ", G/grad_norm: {:.8f}".format(float(host_clip[0]))
                    if host_lr is not None:                       # {rate of the last applied step, rate / base, its t, kind}
                        log += ", lr: {:.8e}".format(float(host_lr[0]))
                    print(log)
                    if host_clip is not None and int(host_clip[3]) > skipped_seen:
                        print('Warning: {} optimiser step(s) skipped so far: their gradients were not finite (by iteration {})'.format(
                            int(host_clip[3]), it))
                        skipped_seen = int(host_clip[3])

        for i in range(start_iters, self.num_iters):
            batch = next(data_iter) if self.accum_steps == 1 else [next(data_iter) for _ in range(self.accum_steps)]
            self.G = self.G.train()
            loss_dev = self.train_on_batch(batch)
            if (i + 1) % self.log_step == 0:
                t = loss_dev
                if self.world > 1:
                    # data parallel: every rank synchronises and checks at the SAME iteration (a rank that noticed a failure an
                    # iteration earlier than the others would leave them waiting in a collective)
                    import torch.distributed as dist
                    torch.cuda.synchronize(self.device)
                    self.eng.check()
                    t = loss_dev.clone()
                    dist.all_reduce(t)
                    t = t / self.world
                elif self.eng.status():                           # host-visible status word, no sync: a persistent kernel that gave up
                    self.eng.check()                              # waiting in an earlier step has said so by now (raises)
                host_loss = torch.empty((), dtype=torch.float32).pin_memory()
                host_loss.copy_(t.reshape(()), non_blocking=True)
                host_clip = None
                if self.grad_clip:                                # the same pinned non-blocking copy as the loss
                    host_clip = torch.empty(4, dtype=torch.float32).pin_memory()
                    host_clip.copy_(self.eng.grad_clip_stats(), non_blocking=True)
                host_lr = None
                if self.lr_schedule:
                    host_lr = torch.empty(4, dtype=torch.float32).pin_memory()
                    host_lr.copy_(self.eng.lr_stats(), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                pending.append((ev, host_loss, i + 1, str(datetime.timedelta(seconds=time.time() - start_time))[:-7], host_clip, host_lr))
            flush(self.world > 1)
            if (i + 1) % self.model_save_step == 0 and self.rank == 0:
                flush(True)
                self.save_model(i + 1)
                print('Saved model checkpoints into {}...'.format(self.model_save_dir))
            if (i + 1) % self.sample_step == 0 and validation_pt is not None and self.rank == 0:
                flush(True)
                val_loss, _ = self.validate(validation_pt)
                print('Validation loss: {}'.format(val_loss))
                if self.eng.ema is not None:
                    val_loss, _ = self.validate(validation_pt, ema=True)
                    print('Validation loss (EMA): {}'.format(val_loss))
        flush(True)
        self.eng.check()                                          # the last steps too (synchronises)


class SolverF0(Solver):
    """Trainer for Generator_6, the F0 converter (reference model.py:324-351; demo.ipynb cell 0 uses a pretrained one, `640000-P.ckpt`).
    The reference ships NO training loop for it: this one is this repo's choice and says so -- the `Solver` shell
    unchanged (constructor, config attributes, log line, `<iter>-G.ckpt` layout with the reference's Generator_6 key names), the step
    body = quantise the batch's F0 (utils.quantize_f0_torch), feed the one-hot as `f0_trg`, cross-entropy of the 257-way logits
    against the same classes (demo.ipynb takes their argmax), backward, Adam: ONE `ss_g6_train_step` call.  BASELINE config 4."""
    GENERATOR = Generator_6

    N_DRAWS = 3                    # Encoder_6 resamples three times (model.py:128)

    def _step(self, batch, draws, last=True, accumulate=False, grad_scale=1.0):
        from .utils import quantize_f0_torch
        (x_real_org, emb_org, f0_org, len_org), draws = self._shard(batch, draws)
        to = dict(device=self.device, non_blocking=True)
        mel, f0 = x_real_org.to(**to), f0_org.to(**to)
        onehot, idx = quantize_f0_torch(f0[:, :, 0])
        bucket = mel.shape[1] != self.hparams.max_len_pad
        args = (mel, onehot, idx.to(torch.int32), draws)
        if not last:
            return self.eng.g6_train_step(*args, no_adam=True, bucket=bucket, accumulate=accumulate)
        if self.world > 1 and self.dp_backend == 'torch':
            return self.eng.dp_g6_train_step(*args, self.world, bucket=bucket, accumulate=accumulate)
        if self.world > 1:
            return self.eng.g6_dp_train_step_native(*args, bucket=bucket, accumulate=accumulate)
        return self.eng.g6_train_step(*args, grad_scale=grad_scale, bucket=bucket, accumulate=accumulate)

    def validate(self, validation_pt, ablations=False, ema=False):
        raise NotImplementedError('the reference validates Generator_3 only (solver.py:206-227)')
