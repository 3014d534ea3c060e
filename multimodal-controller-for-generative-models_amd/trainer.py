"""The train steps, driven directly on the fused engines, and what they step with:

* the fused optimizers (Adam, SGD, RMSprop, Adamax: torch.optim semantics and state_dict format over one flat buffer)
  and the averaged network (``FusedEMA``);
* the GAN step of MCGAN and CGAN (``GANTrainer``; ``GraphedGANTrainer`` replays it from HIP graphs), the counterpart of
  the loop body of the reference's ``train_gan.py:139-176``.  The body is written once (``GANTrainer._step``); the eager
  trainer, the capture warm-up and the one-graph capture call it, the per-bucket capture cuts the same pieces apart;
* the single-network steps (``_FlatTrainer``: Glow, PixelCNN, VAE, VQ-VAE, classifier).

Per data batch: ``d_iters`` (5) discriminator updates -- D(real), G(z) in training mode,
D(G(z).detach()), hinge loss, backward, Adam(D) -- then ``g_iters`` (1) generator updates --
G(z), D(G(z)), -mean, backward through D into G, Adam(G).  Adam(lr 2e-4, betas (0.5, 0.999),
eps 1e-8, no weight decay) as configured at train_gan.py:43-47,231.

The discriminator weight gradient of the generator step, which the reference computes and then
discards at the next zero_grad (train_gan.py:141,163), is skipped.

Data parallel: one process per GPU; each rank runs this step on its shard and the flat gradient
buffer of the network being updated is all-reduced (average) over RCCL before Adam
(``dist_group`` != None).  BatchNorm statistics stay per-rank, as with the reference's
nn.DataParallel (train_gan.py:96-98).
"""
from __future__ import annotations

import contextlib
from typing import Optional, Sequence

import torch
import torch.nn.functional as F

from . import ops
from .gan_engine import FlatState, Nhwc, _bump
from .vae_engine import check_train_batch

# 'thread_local': other threads of the process (the RCCL watchdog of a multi-rank run polls events) may keep
# making HIP calls while this thread captures; only this thread's illegal calls abort the capture.
_CAPTURE_MODE = 'thread_local'

from ._tuning import flag as _flag
_NHWC_PAIR = _flag('MCGEN_NHWC_PAIR', '1') != '0'    # engine-to-engine images stay NHWC (0: through NCHW fp32, as round 1)
_PAIR_D = _flag('MCGEN_PAIR_D', '1') != '0'      # real + fake discriminator passes batched (see d_compute)
_GROUP_G = _flag('MCGEN_GROUP_G', '1') != '0'    # the d_iters generator forwards of an iteration as one pass (fake_groups)
_FUSE_D_ADAM = _flag('MCGEN_FUSE_D_ADAM', '1') != '0'     # single rank: spectral-norm gradient fix + Adam of a paired D update in one launch
_FUSE_TAIL = _flag('MCGEN_FUSE_TAIL', '1') != '0'        # D tail forward + loss derivative + tail input gradient in one launch
_ONE_GRAPH = _flag('MCGEN_ONE_GRAPH', '1') != '0'        # single rank: the whole loop body as one HIP graph (0: one graph per phase, as a multi-rank run)


class _FusedOptimizer:
    """What the fused optimizers share: the learning rate as a device scalar and the step counter's buffer."""

    def _init_buffers(self, flat_state: FlatState, lr) -> torch.Tensor:
        self.fs = flat_state
        flat = self.fs.ensure()
        self._step_buf = torch.zeros(2, dtype=torch.int64, device=flat.device)     # {step counter, launch ticket} (ops.adam)
        self.step_count = self._step_buf[:1]
        # the learning rate lives in device memory and the kernels read it when they run (mcgen_adam's lr_dev): a
        # scheduler step is one fill_ and the captured graphs stay valid
        self._lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=flat.device) if flat.is_cuda else None
        self.lr = lr
        return flat

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        self._lr = float(value)
        if getattr(self, '_lr_dev', None) is not None:
            self._lr_dev.fill_(self._lr)

    def set_lr(self, lr: float):
        self.lr = float(lr)

    def _lr_arg(self):
        return self._lr_dev if self._lr_dev is not None else self._lr


class _FusedTorchState(_FusedOptimizer):
    """state_dict() / load_state_dict() of the fused optimizers in the format of the matching
    torch.optim class (the reference checkpoints optimizer.state_dict(), train_vae.py:85): a subclass names its state
    in `_slots()`, its hyper-parameters in `_group()` and takes a loaded group in `_load_group()`."""
    _has_step = True                     # torch keeps a per-parameter 'step' (SGD does not)

    def _slots(self):                    # [(torch's state key, flat buffer)], in torch's order
        raise NotImplementedError

    def _group(self):                    # torch's param_groups[0] without 'params'
        raise NotImplementedError

    def _load_group(self, g):            # refuse what the kernel does not implement, then take the hyper-parameters
        raise NotImplementedError

    def _momentum_buffer(self):
        """The momentum buffer exists exactly when momentum > 0 (mcgen_sgd / mcgen_rmsprop take NULL otherwise)."""
        if self.momentum == 0:
            self.buf = None
        elif self.buf is None:
            self.buf = torch.zeros_like(self.fs.ensure())
        return self.buf

    def state_tensors(self):
        """The device tensors that make up the optimizer's state: what a capture warm-up snapshots and restores."""
        return [t for _, t in self._slots()] + [self.step_count]

    def _bump_params(self):
        for p in self.fs.tensors:
            _bump(p)

    def state_dict(self):
        """{'state': {i: {...}}, 'param_groups': [...]} over the parameters in `model.parameters()` order; 'state' is
        empty before the first step (and always for SGD without momentum), as torch's is."""
        self.fs.ensure()
        state, slots = {}, self._slots()
        if int(self.step_count) > 0 and (slots or self._has_step):
            step = self.step_count.to(torch.float32).reshape(())
            for i, t in enumerate(self.fs.tensors):
                state[i] = {'step': step.clone()} if self._has_step else {}
                for key, buf in slots:
                    state[i][key] = self.fs.view_of(buf, t).clone()
        return {'state': state, 'param_groups': [dict(self._group(), params=list(range(len(self.fs.tensors))))]}

    def load_state_dict(self, sd):
        self.fs.ensure()
        groups = sd['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != len(self.fs.tensors):
            raise ValueError('Not valid optimizer state: expected one parameter group over the network\'s parameters')
        g = groups[0]
        if g.get('maximize'):
            raise ValueError('Not valid optimizer state: maximize is not supported')
        self._load_group(g)
        for t in self.state_tensors():
            t.zero_()
        steps = set()
        for key, t in zip(g['params'], self.fs.tensors):
            st = sd['state'].get(key)
            if not st:
                continue
            for name, buf in self._slots():
                self.fs.view_of(buf, t).copy_(st[name])
            steps.add(int(st['step']) if self._has_step else 1)     # (SGD: any state means "has stepped")
        if len(steps) > 1:
            raise ValueError('Not valid optimizer state: parameters disagree on the step count')
        if steps:
            self.step_count.fill_(steps.pop())


class FusedAdam(_FusedTorchState):
    """torch.optim.Adam semantics over one flat parameter buffer: one launch per step."""

    def __init__(self, flat_state: FlatState, lr=2e-4, betas=(0.5, 0.999), eps=1e-8, weight_decay=0.0):
        self.betas, self.eps, self.wd = betas, eps, weight_decay
        flat = self._init_buffers(flat_state, lr)
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)

    def hyper(self):
        """The hyper-parameters a launch bakes in as kernel arguments (a captured HIP graph replays the values it was
        captured with: the graphed trainers compare this key on every iteration and re-capture when it moved).  The
        learning rate is NOT among them: it is read from device memory at execution time."""
        return (tuple(float(b) for b in self.betas), float(self.eps), float(self.wd))

    def _slots(self):
        return [('exp_avg', self.m), ('exp_avg_sq', self.v)]

    def step(self, gflat: torch.Tensor):
        flat = self.fs.ensure()
        ops.adam(flat, gflat, self.m, self.v, self._step_buf, self._lr_arg(), self.betas, self.eps, self.wd)
        self._bump_params()

    def step_fused_sn_pair(self, pending):
        """The discriminator's update straight from the raw per-half gradients of a paired pass (DiscriminatorEngine.
        backward_iter(defer_fix=True)): spectral-norm fix + Adam in one launch per layer table (ops.sn_fix_pair_adam)."""
        flat = self.fs.ensure()
        tables = [t for t in pending['tables'] if t[0][1] > 0]
        for i, ((table, nl), sg_off) in enumerate(tables):
            ops.sn_fix_pair_adam(pending['g0'], pending['g1'], flat, self.m, self.v, pending['uv0'], pending['uv1'], table, nl,
                                 pending['sigma0'][sg_off:], pending['sigma1'][sg_off:], self._step_buf, self._lr_arg(), self.betas,
                                 self.eps, self.wd, i == 0)
        self._bump_params()

    # (train_gan.py:114-115,268-269: the reference checkpoints optimizer['generator'].state_dict() and loads it back)
    def _group(self):
        return {'lr': self.lr, 'betas': tuple(self.betas), 'eps': self.eps, 'weight_decay': self.wd, 'amsgrad': False,
                'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
                'decoupled_weight_decay': False}

    def _load_group(self, g):
        if g.get('amsgrad'):
            raise ValueError('Not valid optimizer state: amsgrad is not supported')
        self.lr, self.betas, self.eps, self.wd = g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']

    def load_state_dict(self, sd):
        if 'param_groups' in sd:
            return super().load_state_dict(sd)
        self.fs.ensure()                                 # round-1 private format {'m', 'v', 'step', ...}
        self.m.copy_(sd['m']); self.v.copy_(sd['v']); self.step_count.copy_(sd['step'])
        self.lr, self.betas, self.eps, self.wd = sd['lr'], tuple(sd['betas']), sd['eps'], sd['weight_decay']


class FusedSGD(_FusedTorchState):
    """torch.optim.SGD (momentum, no dampening, no Nesterov) over one flat parameter buffer: one launch per step
    (mcgen_sgd).  momentum = 0 keeps no state at all."""
    _has_step = False

    def __init__(self, flat_state: FlatState, lr=1e-3, momentum=0.0, weight_decay=0.0):
        self.momentum, self.wd, self.buf = momentum, weight_decay, None
        self._init_buffers(flat_state, lr)
        self._momentum_buffer()

    def hyper(self):
        """What a launch bakes in as kernel arguments (see FusedAdam.hyper): not the learning rate."""
        return (float(self.momentum), float(self.wd))

    def _slots(self):
        buf = self._momentum_buffer()
        return [] if buf is None else [('momentum_buffer', buf)]

    def step(self, gflat: torch.Tensor):
        ops.sgd(self.fs.ensure(), gflat, self._momentum_buffer(), self._step_buf, self._lr_arg(), self.momentum, self.wd)
        self._bump_params()

    def _group(self):
        return {'lr': self.lr, 'momentum': self.momentum, 'dampening': 0, 'weight_decay': self.wd, 'nesterov': False,
                'maximize': False, 'foreach': None, 'differentiable': False, 'fused': None}

    def _load_group(self, g):
        if g.get('nesterov') or g.get('dampening', 0) != 0:
            raise ValueError('Not valid optimizer state: nesterov / dampening are not supported')
        self.lr, self.momentum, self.wd = g['lr'], g['momentum'], g['weight_decay']


class FusedRMSprop(_FusedTorchState):
    """torch.optim.RMSprop (not centered) over one flat parameter buffer: one launch per step (mcgen_rmsprop)."""

    def __init__(self, flat_state: FlatState, lr=1e-2, alpha=0.99, eps=1e-8, momentum=0.0, weight_decay=0.0):
        self.alpha, self.eps, self.momentum, self.wd, self.buf = alpha, eps, momentum, weight_decay, None
        flat = self._init_buffers(flat_state, lr)
        self.sq = torch.zeros_like(flat)
        self._momentum_buffer()

    def hyper(self):
        """What a launch bakes in as kernel arguments (see FusedAdam.hyper): not the learning rate."""
        return (float(self.alpha), float(self.eps), float(self.momentum), float(self.wd))

    def _slots(self):
        buf = self._momentum_buffer()
        return [('square_avg', self.sq)] + ([] if buf is None else [('momentum_buffer', buf)])

    def step(self, gflat: torch.Tensor):
        ops.rmsprop(self.fs.ensure(), gflat, self.sq, self._momentum_buffer(), self._step_buf, self._lr_arg(), self.alpha,
                    self.eps, self.momentum, self.wd)
        self._bump_params()

    def _group(self):
        return {'lr': self.lr, 'momentum': self.momentum, 'alpha': self.alpha, 'eps': self.eps, 'centered': False,
                'weight_decay': self.wd, 'capturable': False, 'foreach': None, 'maximize': False, 'differentiable': False}

    def _load_group(self, g):
        if g.get('centered'):
            raise ValueError('Not valid optimizer state: centered is not supported')
        self.lr, self.momentum, self.alpha, self.eps, self.wd = g['lr'], g['momentum'], g['alpha'], g['eps'], g['weight_decay']


class FusedAdamax(_FusedTorchState):
    """torch.optim.Adamax over one flat parameter buffer: one launch per step (mcgen_adamax; `m`: exp_avg, `u`: exp_inf)."""

    def __init__(self, flat_state: FlatState, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.betas, self.eps, self.wd = betas, eps, weight_decay
        flat = self._init_buffers(flat_state, lr)
        self.m = torch.zeros_like(flat)
        self.u = torch.zeros_like(flat)

    def hyper(self):
        """What a launch bakes in as kernel arguments (see FusedAdam.hyper): not the learning rate."""
        return (tuple(float(b) for b in self.betas), float(self.eps), float(self.wd))

    def _slots(self):
        return [('exp_avg', self.m), ('exp_inf', self.u)]

    def step(self, gflat: torch.Tensor):
        ops.adamax(self.fs.ensure(), gflat, self.m, self.u, self._step_buf, self._lr_arg(), self.betas, self.eps, self.wd)
        self._bump_params()

    def _group(self):
        return {'lr': self.lr, 'betas': tuple(self.betas), 'eps': self.eps, 'weight_decay': self.wd, 'foreach': None,
                'maximize': False, 'differentiable': False, 'capturable': False}

    def _load_group(self, g):
        self.lr, self.betas, self.eps, self.wd = g['lr'], tuple(g['betas']), g['eps'], g['weight_decay']


def make_fused_optimizer(name: str, flat_state: FlatState, lr, betas=(0.9, 0.999), momentum=0.0, weight_decay=0.0):
    """The fused counterpart of the reference's make_optimizer (train_gan.py:222-236, train_vae.py:151-165): the same
    arguments reach the same optimizers (momentum: SGD and RMSprop; betas: Adam and Adamax)."""
    if name == 'SGD':
        return FusedSGD(flat_state, lr=lr, momentum=momentum, weight_decay=weight_decay)
    if name == 'RMSprop':
        return FusedRMSprop(flat_state, lr=lr, momentum=momentum, weight_decay=weight_decay)
    if name == 'Adam':
        return FusedAdam(flat_state, lr=lr, betas=betas, weight_decay=weight_decay)
    if name == 'Adamax':
        return FusedAdamax(flat_state, lr=lr, betas=betas, weight_decay=weight_decay)
    raise ValueError('Not valid optimizer name')


def ema_state_dict(decay, start, step, params, buffers):
    """The checkpoint form of an averaged network: {'decay', 'start', 'step', 'params': {name: tensor}, 'buffers':
    {name: tensor}} -- `params` / `buffers`: (name, tensor) pairs, cloned here."""
    return {'decay': float(decay), 'start': int(start), 'step': int(step),
            'params': {k: v.detach().clone() for k, v in params},
            'buffers': {k: v.detach().clone() for k, v in buffers}}


def ema_load_into(sd, params, buffers):
    """Copy an `ema_state_dict` into the (name, tensor) pairs `params` / `buffers`; -> (decay, start, step).  The names and
    shapes must be the dict's own."""
    for kind, pairs in (('params', list(params)), ('buffers', list(buffers))):
        have = sd[kind]
        if set(have) != {k for k, _ in pairs}:
            raise ValueError(f'Not valid averaged state: {kind} do not match the network\'s')
        for k, t in pairs:
            if tuple(have[k].shape) != tuple(t.shape):
                raise ValueError(f'Not valid averaged state: shape of {k}')
            t.copy_(have[k])
    return float(sd['decay']), int(sd['start']), int(sd['step'])


def ema_buffers(module):
    """{name: tensor} of a network's float BatchNorm running statistics, named as in module.state_dict(): what the
    averaged network keeps its own copy of (codebooks and num_batches_tracked are not averaged)."""
    return {k: b for k, b in module.named_buffers()
            if b.is_floating_point() and k.rsplit('.', 1)[-1] in ('running_mean', 'running_var')}


class FusedEMA:
    """An exponential moving average of a network: of its parameters (one FlatState) and of its float BatchNorm running
    statistics, which are flattened here once (the averaged network runs in eval mode on running statistics, so averaged
    weights need averaged statistics).  update() is two launches of mcgen_ema_update -- one when there are no buffers --
    which read the update count from device memory, so a captured update stays valid: update k (from 0) copies while
    k < start and averages with `decay` from then on.  `names`: the parameters' names, in flat_state.tensors order;
    `buffers`: {name: tensor}; `on_swap`: called after the averaged values went into or out of the live tensors."""

    def __init__(self, flat_state: FlatState, buffers, decay: float, start: int = 0, names: Optional[Sequence[str]] = None,
                 on_swap=None):
        if not 0.0 <= float(decay) < 1.0 or int(start) < 0:
            raise ValueError('Not valid averaging: decay in [0, 1) and start >= 0')
        self.decay, self.start = float(decay), int(start)
        self.fs = flat_state
        flat = self.fs.ensure()
        self.names = list(names) if names is not None else [str(i) for i in range(len(self.fs.tensors))]
        assert len(self.names) == len(self.fs.tensors)
        buffers = dict(buffers)
        self.buffer_names = list(buffers)
        self.bfs = FlatState(list(buffers.values())) if buffers else None
        self.avg_p = flat.detach().clone()
        self.avg_b = self.bfs.ensure().detach().clone() if self.bfs is not None else None
        self._step_buf = torch.zeros(2, dtype=torch.int64, device=flat.device)     # {update counter, launch ticket} (ops.adam)
        self.step_count = self._step_buf[:1]
        self.on_swap = on_swap

    def hyper(self):
        """(decay, start): kernel arguments of the update launches -- a captured graph replays the values it was captured
        with, so the graphed trainers treat a change like an optimizer-hyper change (FusedAdam.hyper)."""
        return (self.decay, self.start)

    def state_tensors(self):
        """The device tensors that make up the state: what a capture warm-up snapshots and restores."""
        return [self.avg_p] + ([self.avg_b] if self.avg_b is not None else []) + [self.step_count]

    def update(self):
        flat = self.fs.ensure()
        if self.bfs is None:
            ops.ema_update(self.avg_p, flat, self._step_buf, self.decay, self.start, advance=True)
            return
        # the count advances once per update: on the last launch
        ops.ema_update(self.avg_p, flat, self._step_buf, self.decay, self.start, advance=False)
        ops.ema_update(self.avg_b, self.bfs.ensure(), self._step_buf, self.decay, self.start, advance=True)

    def _swap(self):
        ops.swap_(self.avg_p, self.fs.ensure())
        if self.bfs is not None:
            ops.swap_(self.avg_b, self.bfs.ensure())
        for t in self.fs.tensors + (self.bfs.tensors if self.bfs is not None else []):
            _bump(t)
        if self.on_swap is not None:
            self.on_swap()

    @contextlib.contextmanager
    def swapped(self):
        """Inside the context the live tensors hold the averaged values (and the average's buffers the live ones): an
        in-place exchange, no pointer a captured graph holds moves.  Every swapped tensor's version is bumped both times."""
        self._swap()
        try:
            yield self
        finally:
            self._swap()

    def _named(self):
        params = list(zip(self.names, self.fs.views(self.avg_p)))
        buffers = list(zip(self.buffer_names, self.bfs.views(self.avg_b))) if self.bfs is not None else []
        return params, buffers

    def state_dict(self):
        """{'decay', 'start', 'step', 'params': {name: tensor}, 'buffers': {name: tensor}} (ema_state_dict)."""
        self.fs.ensure()
        params, buffers = self._named()
        return ema_state_dict(self.decay, self.start, int(self.step_count), params, buffers)

    def load_state_dict(self, sd):
        self.fs.ensure()
        params, buffers = self._named()
        self.decay, self.start, step = ema_load_into(sd, params, buffers)
        self.step_count.fill_(step)

    def reset(self):
        """Start the average over from the current parameters and statistics (a resume from a file without one)."""
        self.avg_p.copy_(self.fs.ensure())
        if self.bfs is not None:
            self.avg_b.copy_(self.bfs.ensure())
        self._step_buf.zero_()


class FusedLeCam:
    """The device state of the LeCam regulariser of the discriminator loss (include/mcgen_hip.h, mcgen_lecam_state_t):
    the anchors a_R / a_F (running means of the real / generated logits), the count t of discriminator updates and the
    last update's statistics, as ONE int64 tensor the kernels address, with float32 / int64 views over it.  The launches
    that form the discriminator loss read and move it (ops.dtail_lecam_fused + ops.dtail_pair_wgrad(lecam=...) on the
    paired path, ops.lecam_loss_d elsewhere): nothing here launches anything, and t lives on the device, so a captured
    update stays valid.  `lam` > 0: the term lam * R is on from update `start`; the anchors move from update 0."""

    def __init__(self, device, lam: float, decay: float = 0.99, start: int = 0):
        self.lam, self.decay, self.start = self.check_hyper(lam, decay, start)
        words, self._f, self._t = ops.lecam_state_layout()
        self.state = torch.zeros(words, dtype=torch.int64, device=device)
        self._floats = self.state.view(torch.float32)
        self.step_count = self.state[self._t:self._t + 1]

    @staticmethod
    def check_hyper(lam, decay, start):
        lam, decay, start = float(lam), float(decay), int(start)
        if not (0.0 <= lam < float('inf')) or not 0.0 <= decay < 1.0 or start < 0:
            raise ValueError('Not valid LeCam regulariser: lambda >= 0 and finite, decay in [0, 1) and start >= 0')
        return lam, decay, start

    def hyper(self):
        """(lambda, decay, start): kernel arguments of the loss launches, baked into a captured graph (FusedEMA.hyper)."""
        return (self.lam, self.decay, self.start)

    def state_tensors(self):
        return [self.state]

    def anchors(self):
        """(a_R, a_F) as device scalars: views, they follow the updates."""
        return self._floats[self._f['a_real']], self._floats[self._f['a_fake']]

    def stats(self):
        """Of the last discriminator update, device scalars: the mean real / generated logit, r_t = mean sign(D(real))
        (ADA's overfitting indicator) and the regulariser's value R (before lambda)."""
        f = self._floats
        return {'m_R': f[self._f['m_real']], 'm_F': f[self._f['m_fake']], 'r_t': f[self._f['r_t']], 'R': f[self._f['reg']]}

    def state_dict(self):
        a_r, a_f = self.anchors()
        return {'lambda': self.lam, 'decay': self.decay, 'start': self.start, 'a_R': float(a_r), 'a_F': float(a_f),
                'step': int(self.step_count), 'stats': {k: float(v) for k, v in self.stats().items()}}

    def load_state_dict(self, sd):
        """Takes the anchors, the count and the statistics; the hyper-parameters stay the constructor's (they are the
        flags of THIS run, and a captured graph holds them) -- where the dict's differ, a line says so."""
        theirs = tuple(sd.get(k) for k in ('lambda', 'decay', 'start'))
        if all(v is not None for v in theirs) and (float(theirs[0]), float(theirs[1]), int(theirs[2])) != self.hyper():
            print('LeCam state was accumulated with (lambda, decay, start) = {}; this run goes on with {}'.format(theirs, self.hyper()))
        host = torch.zeros(self.state.numel(), dtype=torch.int64)
        f = host.view(torch.float32)
        f[self._f['a_real']], f[self._f['a_fake']] = float(sd['a_R']), float(sd['a_F'])
        for k, field in (('m_R', 'm_real'), ('m_F', 'm_fake'), ('r_t', 'r_t'), ('R', 'reg')):
            f[self._f[field]] = float(sd.get('stats', {}).get(k, 0.0))
        host[self._t] = int(sd['step'])
        self.state.copy_(host)

    def reset(self):
        self.state.zero_()


def _graph(fn, pool=None):
    """`fn()` captured into a new HIP graph (in the memory pool of an earlier one, if given)."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, pool=pool, capture_error_mode=_CAPTURE_MODE):
        fn()
    return g


def _rehearse(model, stateful, body, times: int, settle):
    """A capture's warm-up, rolled back: `times` runs of `body` on a side stream, then model.state_dict() and the
    state_tensors() of the `stateful` objects go back to what they were and `settle()` re-derives what follows them.  So a
    capture leaves the model, the optimizer state and every buffer as it found them (the capture itself records launches,
    it does not execute them)."""
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    saved = [[t.clone() for t in o.state_tensors()] for o in stateful]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(max(1, times)):
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():
        model.load_state_dict(sd)
        for o, ts in zip(stateful, saved):
            for t, s in zip(o.state_tensors(), ts):
                t.copy_(s)
    settle()
    torch.cuda.synchronize()


class GANTrainer:
    def __init__(self, model, classes: int, lr=2e-4, betas=(0.5, 0.999), d_iters: int = 5, g_iters: int = 1,
                 dist_group=None, world_size: int = 1, grad_wire_dtype: Optional[torch.dtype] = None,
                 optimizer: str = 'Adam', momentum: float = 0.0, weight_decay: float = 0.0,
                 ema_decay: float = 0.0, ema_start: int = 0, loss_type: str = 'Hinge',
                 lecam_lambda: float = 0.0, lecam_decay: float = 0.99, lecam_start: int = 0):
        # the LeCam regulariser of the D loss (FusedLeCam; off at 0: then no launch, argument or result differs).  Checked
        # before anything touches a device.
        lecam_hyper = FusedLeCam.check_hyper(lecam_lambda, lecam_decay, lecam_start)
        if lecam_hyper[0] > 0 and world_size > 1:
            raise ValueError('Not valid LeCam regulariser: lecam_lambda > 0 runs on one GPU -- each rank would keep anchors of '
                             'its own shard of the batch; anchors shared between ranks are not implemented')
        self.model = model
        # cfg['loss_type'] of train_gan.py:55,148-156,168-174; fixed here: a captured graph bakes its launches in
        ops.gan_loss_id(loss_type)                        # (raises the reference's ValueError('Not valid loss type'))
        self.loss_type = loss_type
        self.grad_wire_dtype = grad_wire_dtype            # torch.bfloat16: gradient buckets cross the links as bf16 (dist.allreduce_mean_)
        self._ov = None                                   # overlap bookkeeping (overlap_begin / overlap_end)
        self.classes = classes
        self.d_iters, self.g_iters = d_iters, g_iters
        self.geng = model.generator._engine()
        self.deng = model.discriminator._engine()
        self.geng.flat_p.ensure()
        self.deng._ensure_flat()
        # cfg['optimizer_name'] of train_gan.py:222-236: both networks take the same optimizer, as in the reference
        self.opt_g = make_fused_optimizer(optimizer, self.geng.flat_p, lr, betas, momentum, weight_decay)
        self.opt_d = make_fused_optimizer(optimizer, self.deng.flat_p, lr, betas, momentum, weight_decay)
        self.grad_g = torch.zeros_like(self.geng.flat_p.flat)
        self.grad_d = torch.zeros_like(self.deng.flat_p.flat)
        self.group, self.world = dist_group, world_size
        self.latent = model.latent_size
        # CGAN (models/cgan.py): labels go to the engines' embedding kernels; no codes, no paired D pass (see _CGANPieces)
        self._cgan = bool(getattr(model, 'label_embedding', False))
        if self._cgan and world_size > 1:
            raise ValueError('CGAN training runs on one GPU: its gradients are not bucketed for a data-parallel exchange')
        self._pieces = (_CGANPieces if self._cgan else _MCGANPieces)(self)      # the model's parts of the step (_step)
        # the averaged generator (opt-in): updated right behind every generator optimizer step (g_apply).  A multi-rank run
        # needs no exchange for it: every rank averages the same parameters.
        self.lecam = None
        if lecam_hyper[0] > 0:
            self.lecam = FusedLeCam(self.grad_d.device, *lecam_hyper)
        self.ema = None
        if ema_decay:
            gen = model.generator
            name_of = {id(p): k for k, p in gen.named_parameters()}
            self.ema = FusedEMA(self.geng.flat_p, ema_buffers(gen), ema_decay, ema_start,
                                names=[name_of[id(p)] for p in self.geng.flat_p.tensors],
                                on_swap=lambda: self.geng.refresh_images(force=True))

    def ema_weights(self):
        """Context manager: inside it the generator holds its averaged parameters and running statistics (for scoring and
        sampling in eval mode).  The weight images are rebuilt eagerly on entry AND on exit: a replayed compute graph does
        not look at the image cache, so the live weights' images must be back before the next replay."""
        if self.ema is None:
            raise ValueError('Not valid averaging: the trainer was built with ema_decay = 0')
        return self.ema.swapped()

    def _hyper(self):
        """What the captured launches bake in (see FusedAdam.hyper, FusedEMA.hyper)."""
        key = (self.opt_g.hyper(), self.opt_d.hyper(), self.loss_type)
        if self.ema is not None:
            key += (self.ema.hyper(),)
        return key if self.lecam is None else key + (('lecam',) + self.lecam.hyper(),)      # (last: train_iteration looks there)

    def _loss_d(self, real, fake, both=False):
        """The stand-alone D loss of the legs without the fused tail (and of CGAN's two passes): ops.gan_loss_d, or with the
        LeCam regulariser on ops.lecam_loss_d, which also moves the holder's state -- one launch either way."""
        if self.lecam is None:
            return ops.gan_loss_d(real, fake, self.loss_type, both=both)
        lc = self.lecam
        return ops.lecam_loss_d(real, fake, self.loss_type, lc.state, lc.lam, lc.decay, lc.start, both=both)

    # ---- data-parallel gradient exchange: two buckets per network, started under the backward pass -------------
    # The engines' backward passes hand out each network's flat gradient in two contiguous buckets: the LATE layers
    # (tail / head + the late residual blocks), final when about half of the backward is done, and the early layers at
    # its end (gan_engine: backward_iter, bucket_cut).  A bucket's all-reduce (average, RCCL over xGMI) is launched on
    # a communication stream the moment it is final, so the late bucket's exchange runs under the rest of the backward
    # pass; the optimizer step waits for both.  (train_gan.py:96-98: the reference's nn.DataParallel sums replica
    # gradients onto device 0 after the whole backward.)
    def _comm_stream(self):
        cs = getattr(self, '_comm', None)
        if cs is None:
            cs = self._comm = torch.cuda.Stream()
        return cs

    def _reduce_bucket(self, g: torch.Tensor, lo: int, hi: int):
        if self.world > 1 and hi > lo:
            from .dist import allreduce_mean_
            cs = self._comm_stream()
            cs.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(cs):
                if self._ov is not None:
                    e0 = torch.cuda.Event(enable_timing=True); e0.record(cs)
                allreduce_mean_(g[lo:hi], self.world, self.group, self.grad_wire_dtype)
                if self._ov is not None:
                    e1 = torch.cuda.Event(enable_timing=True); e1.record(cs)
                    self._ov['pending'].append((e0, e1))

    def _join_comm(self):
        if self.world > 1:
            if self._ov is not None:
                j = torch.cuda.Event(enable_timing=True); j.record(torch.cuda.current_stream())
                self._ov['joins'].append((j, self._ov['pending'])); self._ov['pending'] = []
            torch.cuda.current_stream().wait_stream(self._comm_stream())

    # ---- how much of the gradient exchange runs under the backward pass ----------------------------------------------
    def overlap_begin(self):
        """Start timing every bucket's all-reduce (events on the communication stream) against the moment the compute
        stream reaches the join in front of the optimizer step."""
        self._ov = {'pending': [], 'joins': []}

    def overlap_end(self):
        """-> {'comm_us': time the all-reduces ran, 'overlap_us': the part of it that ran while the compute stream was
        still busy with the rest of the backward pass (hidden), 'exposed_us': the rest}, summed over the iterations since
        overlap_begin()."""
        torch.cuda.synchronize()
        ov, self._ov = self._ov, None
        comm = hidden = 0.0
        for j, pend in (ov['joins'] if ov else []):
            for e0, e1 in pend:
                dur = e0.elapsed_time(e1) * 1e3
                before_join = e0.elapsed_time(j) * 1e3               # < 0: the bucket started after compute reached the join
                comm += dur
                hidden += max(0.0, min(dur, before_join))
        return {'comm_us': comm, 'overlap_us': hidden, 'exposed_us': comm - hidden}

    # ---- the generator passes of the discriminator updates -----------------------------------------
    def fake_groups(self, n: int) -> int:
        """How many of the d_iters generator forwards of an iteration run as ONE pass.  The generator's weights do not
        change between the discriminator updates (train_gan.py:139-158), so G(z_1) ... G(z_5) is one forward over
        5 N images with BatchNorm statistics kept per N-image group (GeneratorEngine.forward, groups): the 4x4 / 8x8 /
        16x16 layers see five times the pixels per launch.  1 when the batch is too small for a tile to stay inside one
        group (then each update runs its own forward, as the reference does)."""
        if _GROUP_G and self.d_iters > 1 and self.geng.groups_supported(n * self.d_iters, self.d_iters):
            return self.d_iters
        return 1

    def g_fakes(self, ind_rep, z_cat, groups: int, nhwc: bool = False, pair_out: Optional[torch.Tensor] = None):
        """Training-mode generator forward(s) for `groups` discriminator updates: [groups * N, C, H, W], detached
        (`nhwc`: as the engines' own `Nhwc`, for `pair_buffers`).  `pair_out` (the buffer of `pair_buffers`): the generated
        batches are written straight into the second halves of its `groups` paired 2N batches and nothing is returned."""
        fake, _ = self.geng.forward(z_cat, ind_rep, True, groups=groups, nhwc=nhwc, one_hot=True, pair_out=pair_out)   # ind_rep comes from F.one_hot
        return fake

    # The real batch is the same for the d_iters updates of an iteration and the generated batches come out of the generator
    # engine in the discriminator engine's layout: the 2N batches of the paired updates are assembled in that layout -- one
    # buffer of `groups` [real (+) generated] batches; the real half is converted once per iteration and replicated, the
    # generated halves are written in place by the generator's image head (mcgen_conv_t.y_group): no copy per update.
    def pair_buffers(self, img: torch.Tensor, groups: int = 1):
        """-> (buffer [groups * 2N, H, W, 8], [`Nhwc` view of paired batch j]) with `img` (NCHW fp32) in every first half."""
        n, c, h, w = img.shape
        dt = self.deng.dtype
        shape = (groups * 2 * n, h, w, ops.pad8(c))
        buf = getattr(self, '_x2', None)
        if buf is None or tuple(buf.shape) != shape or buf.dtype != dt or buf.device != img.device:
            buf = self._x2 = torch.empty(shape, dtype=dt, device=img.device)
        ops.to_nhwc(img.detach().contiguous(), dt, out=buf[:n])
        if groups > 1:
            v = buf.view(groups, 2 * n, h, w, shape[-1])
            v[1:, :n].copy_(v[0, :n].unsqueeze(0).expand(groups - 1, -1, -1, -1, -1))
        return buf, [Nhwc(buf[j * 2 * n:(j + 1) * 2 * n], c) for j in range(groups)]

    def indicators(self, label: torch.Tensor, groups: int, out: Optional[torch.Tensor] = None, lab32: Optional[torch.Tensor] = None):
        """F.one_hot(label, classes).float() (mcgan.py:196,201) max(2, groups) times back to back, ONE launch: the
        indicator of the batch, of the paired 2N batch and of the grouped generator pass are prefixes of it.
        -> (ind [N], ind2 [2N], ind_rep [groups * N])"""
        n = label.shape[0]
        reps = max(2, groups)
        if label.is_cuda:
            if lab32 is None:
                lab32 = torch.empty(reps * n, dtype=torch.int32, device=label.device)
            allr = ops.onehot_rep(label, self.classes, reps, out=out, lab32=lab32)
        else:
            allr, lab32 = F.one_hot(label, self.classes).float().repeat(reps, 1), None
        # the engines may gather codebook rows by label instead of multiplying through every mode (ops.onehot_hint)
        return (ops.onehot_hint(allr[:n], label, 1), ops.onehot_hint(allr[:2 * n], label, 2),
                ops.onehot_hint(allr[:groups * n], label, groups, None if lab32 is None else lab32[:groups * n]))

    # compute = forward + backward into the flat gradient buffer; apply = Adam (+ weight images).
    # The *_iter forms are generators: they yield (lo, hi, last) whenever grad[lo:hi] is final (see _reduce_bucket).
    def d_compute_iter(self, img, ind, fake, ind2=None, x2=None, codes=None, fuse=False):
        """`fake`: this update's generated batch (NCHW fp32, detached).  `ind2` (optional): the indicator twice,
        [2N, modes] -- constant over the D updates of an iteration, so the caller builds it once.  `x2` (optional, instead
        of img / fake): one paired batch of `pair_buffers`, real (+) fake."""
        if x2 is not None and not _PAIR_D:
            n = x2.t.shape[0] // 2
            img, fake, x2 = Nhwc(x2.t[:n], x2.c), Nhwc(x2.t[n:], x2.c), None
        if _PAIR_D:
            # D(real) and D(fake) as one pass over the 2N batch (DiscriminatorEngine.forward_pair): the spectral-norm
            # power iterations of the two reference forwards depend on the weights alone and run first, in order
            logits, ctx = self.deng.forward_pair(img, fake, ind, ind2, x2=x2, codes=codes, tail_loss='d_pair' if _FUSE_TAIL else None,
                                                 loss_type=self.loss_type, lecam=self.lecam)
            n = ind.shape[0]
            lg = logits.view(-1)
            if 'tail' in ctx:
                # the tail's launch formed d(D loss)/d(logit) and the tail's input gradient; the loss value comes out of the
                # backward pass's tail-gradient launch (two launches where there were four)
                self.loss_d, dboth = ctx['loss'][0], ctx['tail'][0]
            else:
                self.loss_d, _, _, dboth = self._loss_d(lg[:n], lg[n:], both=True)      # d(real) and d(fake) side by side
            # `fuse` (single rank): the raw per-half gradients stay as they are -- d_apply turns them into the update in one
            # fused launch per layer table (spectral-norm fix + Adam) and self.grad_d is not written
            yield from self.deng.backward_iter(ctx, dboth, self.grad_d, False, False, split=self.world > 1,
                                               defer_fix=fuse and self.world == 1)
            return
        d_real, ctx_r = self.deng.forward(img, ind, True)
        d_fake, ctx_f = self.deng.forward(fake, ind, True)
        self.loss_d, dreal, dfake = self._loss_d(d_real.view(-1), d_fake.view(-1))
        self.deng.backward(ctx_r, dreal, self.grad_d, False, False)
        yield from self.deng.backward_iter(ctx_f, dfake, self.grad_d, True, False, split=self.world > 1)   # final once the second pass added

    def d_compute(self, img, ind, fake, ind2=None, x2=None, codes=None):
        for _ in self.d_compute_iter(img, ind, fake, ind2, x2, codes):
            pass
        return self.loss_d

    def d_apply(self):
        pending = self.deng.pending_fix
        if pending is not None:
            self.deng.pending_fix = None
            self.opt_d.step_fused_sn_pair(pending)
        else:
            self.opt_d.step(self.grad_d)

    def g_compute_iter(self, ind, z):
        fake, gctx = self.geng.forward(z, ind, True, nhwc=_NHWC_PAIR)  # (engine to engine: images and their gradient stay NHWC)
        d_fake, dctx = self.deng.forward(fake, ind, True, tail_loss='g' if _FUSE_TAIL else None, loss_type=self.loss_type)
        self.loss_g, dfake = ops.gan_loss_g(d_fake.view(-1), self.loss_type)
        if 'tail' in dctx:
            dfake = dctx['tail'][0]                      # (the same values; the tail's input gradient exists already)
        dimg = self.deng.backward(dctx, dfake, None, False, True)
        yield from self.geng.backward_iter(gctx, dimg, self.grad_g, False, split=self.world > 1)

    def g_compute(self, ind, z):
        for _ in self.g_compute_iter(ind, z):
            pass
        return self.loss_g

    def g_apply(self):
        self.opt_g.step(self.grad_g)
        if self.ema is not None:
            self.ema.update()
        self.geng.refresh_images(force=True)

    @property
    def _fuse_d(self) -> bool:
        """The one-launch spectral-norm fix + update of a paired D pass exists for Adam only: any other optimizer takes
        the fixed gradient from grad_d (the route a multi-rank run takes)."""
        return _FUSE_D_ADAM and hasattr(self.opt_d, 'step_fused_sn_pair')

    def d_update(self, img, ind, fake, ind2=None, x2=None, codes=None):
        for lo, hi, _last in self.d_compute_iter(img, ind, fake, ind2, x2, codes, fuse=self._fuse_d):
            self._reduce_bucket(self.grad_d, lo, hi)
        self._join_comm()
        self.d_apply()
        return self.loss_d

    def g_update(self, ind, z):
        for lo, hi, _last in self.g_compute_iter(ind, z):
            self._reduce_bucket(self.grad_g, lo, hi)
        self._join_comm()
        self.g_apply()
        return self.loss_g

    def train_iteration(self, img: torch.Tensor, label: torch.Tensor, zs: Optional[Sequence[torch.Tensor]] = None):
        """One reference loop body on one batch.  `zs`: d_iters + g_iters latent batches to inject
        (parity runs); drawn on the device when None.  Returns (D_loss, G_loss) device scalars of the
        last D and G update, as the reference logs them (train_gan.py:177)."""
        self.model.train(True)
        n = img.shape[0]
        zi = iter(zs) if zs is not None else None
        one = (lambda: next(zi)) if zi is not None else (lambda: torch.randn(n, self.latent, device=img.device))
        return self._step(img, label, lambda count: torch.cat([one() for _ in range(count)]) if count > 1 else one())

    def _step(self, img, label, draw, statics=None):
        """The loop body, written once: the eager iteration, the capture warm-up and the one-graph capture are this function;
        the per-bucket capture cuts the same pieces apart where the body reduces a bucket (GraphedGANTrainer.capture).
        `draw(count)` -> the next `count` latent batches as one [count * N, latent] tensor; `statics`: see
        `_MCGANPieces.stage`.  Returns (D_loss, G_loss) of the last updates."""
        p = self._pieces
        fg = self.fake_groups(img.shape[0])
        inputs = p.stage(img, label, fg, statics)
        for k in range(self.d_iters):
            if k % fg == 0:
                p.fake_pass(inputs, draw(fg))
            for lo, hi, _last in p.d_compute_iter(inputs, k % fg, self._fuse_d):
                self._reduce_bucket(self.grad_d, lo, hi)
            self._join_comm()
            self.d_apply()
        for _ in range(self.g_iters):
            for lo, hi, _last in p.g_compute_iter(inputs, draw(1)):
                self._reduce_bucket(self.grad_g, lo, hi)
            self._join_comm()
            self.g_apply()
        return self.loss_d, self.loss_g


class _MCGANPieces:
    """MCGAN's parts of the step (GANTrainer._step): MultimodalController indicators and codes, and D(real) with D(fake) as one
    paired pass.  The `_NHWC_PAIR = 0` / `_PAIR_D = 0` legs live here and in GANTrainer.d_compute_iter, nowhere else."""
    bucketed = True                      # the compute generators yield gradient buckets: a data-parallel run exchanges them

    def __init__(self, trainer):
        self.t = trainer

    def statics(self, img, fg):
        """The persistent buffers a capture stages into: the indicators (of the batch / of the paired 2N batch / of the
        generator pass: prefixes of one buffer), their int32 labels and, on the NCHW leg, the generated batches.  (The
        paired batches are persistent as they are: pair_buffers keeps its buffer.)"""
        n, reps = img.shape[0], max(2, fg)
        s = {'indall': torch.empty((reps * n, self.t.classes), dtype=torch.float32, device=img.device),
             'lab32': torch.empty(reps * n, dtype=torch.int32, device=img.device)}
        if not _NHWC_PAIR:
            s['fakes'] = img.new_empty((fg * n,) + tuple(img.shape[1:]))
        return s

    def stage(self, img, label, fg, statics=None):
        """The iteration's inputs in the engines' layouts.  `statics` (self.statics(), a capture): where to put them; None
        allocates."""
        t, s = self.t, statics or {}
        ind, ind2, ind_rep = t.indicators(label, fg, out=s.get('indall'), lab32=s.get('lab32'))
        # real (+) generated batches of the fg discriminator updates that share a generator pass
        xbuf, x2s = t.pair_buffers(img, fg) if _NHWC_PAIR else (None, None)
        codes = t.deng.pair_codes(ind2) if (_NHWC_PAIR and _PAIR_D) else None     # the labels' codes: once for the d_iters updates
        return {'img': img, 'ind': ind, 'ind2': ind2, 'ind_rep': ind_rep, 'xbuf': xbuf, 'x2s': x2s, 'codes': codes,
                'fakes': None, 'fakes_buf': s.get('fakes'), 'fg': fg}

    def fake_pass(self, inputs, z_cat):
        """The generator forwards of `fg` discriminator updates: into the paired batches' second halves, or NCHW."""
        i = inputs
        fakes = self.t.g_fakes(i['ind_rep'], z_cat, i['fg'], nhwc=i['xbuf'] is not None, pair_out=i['xbuf'])
        if i['xbuf'] is None:
            keep = i['fakes_buf']                     # (a capture: the D graphs of every pass read the persistent buffer)
            i['fakes'] = fakes if keep is None else keep.copy_(fakes)

    def d_compute_iter(self, inputs, j, fuse):
        i = inputs
        if i['x2s'] is not None:
            return self.t.d_compute_iter(None, i['ind'], None, i['ind2'], x2=i['x2s'][j], codes=i['codes'], fuse=fuse)
        n = i['img'].shape[0]
        return self.t.d_compute_iter(i['img'], i['ind'], i['fakes'][j * n:(j + 1) * n], i['ind2'], fuse=fuse)

    def g_compute_iter(self, inputs, z):
        return self.t.g_compute_iter(inputs['ind'], z)


class _CGANPieces:
    """CGAN's parts of the step, on label-embedding engines (cgan_engine.py).  D(real) and D(fake) are two passes, each with
    its own power iteration, as in the reference (MCGAN's paired pass folds the sigma ratio into its MultimodalController
    codes, which CGAN does not have); the d_iters generator forwards still run as one grouped pass with per-group BatchNorm
    statistics.  Gradients come whole, not in buckets: one GPU, and a capture is always one graph."""
    bucketed = False

    def __init__(self, trainer):
        self.t = trainer

    def statics(self, img, fg):
        return None                          # (one graph: what stage() allocates under the capture stays the graph's)

    def stage(self, img, label, fg, statics=None):
        label_rep = label.repeat(fg) if fg > 1 else label
        real = Nhwc(ops.to_nhwc(img.detach().contiguous(), self.t.deng.dtype), img.shape[1])
        return {'label': label, 'label_rep': label_rep, 'real': real, 'fakes': None, 'fg': fg}

    def fake_pass(self, inputs, z_cat):
        inputs['fakes'], _ = self.t.geng.forward(z_cat, None, True, groups=inputs['fg'], nhwc=True, label=inputs['label_rep'])

    def d_compute_iter(self, inputs, j, fuse):
        t, label, fakes = self.t, inputs['label'], inputs['fakes']
        n = label.shape[0]
        d_real, ctx_r = t.deng.forward(inputs['real'], None, True, label=label)
        d_fake, ctx_f = t.deng.forward(Nhwc(fakes.t[j * n:(j + 1) * n], fakes.c), None, True, label=label)
        t.loss_d, dreal, dfake = t._loss_d(d_real.view(-1), d_fake.view(-1))
        # (the fake pass first: its transposed weight images are the current ones; the sum is the same either way)
        t.deng.backward(ctx_f, dfake, t.grad_d, False, False)
        t.deng.backward(ctx_r, dreal, t.grad_d, True, False)
        yield 0, t.grad_d.numel(), True

    def g_compute_iter(self, inputs, z):
        t, label = self.t, inputs['label']
        fake, gctx = t.geng.forward(z, None, True, nhwc=True, label=label)
        d_fake, dctx = t.deng.forward(fake, None, True, tail_loss='g' if _FUSE_TAIL else None, label=label,
                                      loss_type=t.loss_type)
        t.loss_g, dfake = ops.gan_loss_g(d_fake.view(-1), t.loss_type)
        if 'tail' in dctx:
            dfake = dctx['tail'][0]
        dimg = t.deng.backward(dctx, dfake, None, False, True)
        t.geng.backward(gctx, dimg, t.grad_g, False)
        yield 0, t.grad_g.numel(), True


class GraphedGANTrainer(GANTrainer):
    """Same step (`_step`), captured once into HIP graphs and replayed: the step is a few hundred short
    launches, so replay removes the host launch cost.  On one GPU the body is ONE graph; otherwise it is cut into
    graphs per piece and gradient bucket (`_capture_buckets`), so that the gradient all-reduce of a multi-rank run
    sits BETWEEN replays, on the same stream, and no collective is ever captured.  The latent refresh is a graph of
    its own either way, so that a parity run can inject latents (`zs`) into the very replays the benchmark times.

    `capture` leaves the model, the optimizer state and every buffer exactly as it found them: its warm-up
    iterations are rolled back before the capture (`_rehearse`)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._graphs = None

    # ---- device-side snapshot: every tensor a train iteration writes, restored by a handful of flat copies ----------
    # (bench.py re-loads the initial training state every few iterations so that the discriminator never saturates on
    # the synthetic data: a saturated hinge loss makes every discriminator backward pass multiply all-zero gradients.)
    def _state_tensors(self):
        ts = [self.geng.flat_p.ensure()] + self.opt_g.state_tensors() + self.opt_d.state_tensors()
        ts += list(self.deng._ensure_flat())
        ts += [b for b in self.model.generator.buffers() if b.dtype != torch.int64 or b.dim() == 0]
        if self.ema is not None:
            ts += self.ema.state_tensors()
        if self.lecam is not None:
            ts += self.lecam.state_tensors()
        seen, out = set(), []
        for t in ts:                                  # (codebooks are buffers too: constant, copied all the same; aliases once)
            if t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                out.append(t)
        return out

    def device_snapshot(self):
        live = self._state_tensors()
        return live, [t.detach().clone() for t in live]

    def device_restore(self, snap):
        live, saved = snap
        with torch.no_grad():
            torch._foreach_copy_(live, saved)
        for t in live:
            _bump(t)
        self.geng.refresh_images(force=True)          # G's weight images follow its parameters (D's are rebuilt per pass)

    def _stateful(self):
        """The optimizers, and the averaged generator and the LeCam state when there are any: what moves with a step besides
        the model."""
        return (self.opt_g, self.opt_d) + tuple(o for o in (self.ema, self.lecam) if o is not None)

    def _settle(self):
        """What follows a restored state_dict: the flat buffers, G's weight images, the codebooks' caches."""
        self.geng.flat_p.ensure()
        self.deng._ensure_flat()
        self.geng.refresh_images(force=True)
        self.geng.warm_caps()                       # (load_state_dict bumped the codebooks' versions)

    def _static_draw(self):
        """-> draw(count) for `_step` over the latent buffer: consecutive slices, so the body's order is the layout."""
        n, at = self.s_img.shape[0], [0]

        def draw(count):
            at[0] += count * n
            return self.s_zall[at[0] - count * n:at[0]]
        return draw

    def capture(self, img: torch.Tensor, label: torch.Tensor, warmup: int = 1):
        p, n = self._pieces, img.shape[0]
        fg = self._fg = self.fake_groups(n)
        passes = (self.d_iters + fg - 1) // fg                  # generator passes of the D updates, fg latent batches each
        self.s_img, self.s_label = img.clone(), label.clone()
        # the iteration's latents in the body's order: fg batches per generator pass, then one per generator update
        self.s_zall = torch.randn((passes * fg + self.g_iters) * n, self.latent, device=img.device)
        statics = self._statics = p.statics(self.s_img, fg)    # (kept: the graphs write them on every replay)
        self.model.train(True)

        def body():
            self._step(self.s_img, self.s_label, self._static_draw(), statics)

        _rehearse(self.model, self._stateful(), body, warmup, self._settle)
        if not p.bucketed or (self.world == 1 and _ONE_GRAPH and fg == self.d_iters and self.g_iters == 1):
            # Single rank: nothing sits between the replays (no collective), so the whole loop body is ONE graph -- input
            # staging, the 5 N generator pass, the d_iters discriminator updates (compute, fused fix + Adam) and the
            # generator update -- behind a small graph that redraws the latents (kept apart so that a parity run can inject
            # them).  The ~15 graph launches per iteration of the bucketed form cost ~8.5 us of idle device time each.
            self.g_all = _graph(body)
            self.g_draw = _graph(self.s_zall.normal_, self.g_all.pool())
        else:
            self.g_all = None
            self._capture_buckets(statics, fg, passes)
        self._graphs = True
        self._hyper_key = self._hyper()

    def _capture_buckets(self, statics, fg, passes):
        """The body's pieces as graphs of their own, cut where `_step` reduces a bucket or draws latents: a graph per
        generator pass (the first stages the inputs), per gradient bucket, per optimizer step and per latent draw, so that
        the all-reduces of a multi-rank run sit BETWEEN replays and no collective is ever captured."""
        p, draw = self._pieces, self._static_draw()
        zd = [draw(fg) for _ in range(passes)]
        zg = [draw(1) for _ in range(self.g_iters)]

        def staged_pass():
            # (set while capturing, kept afterwards: the later graphs read these tensors, `codes` among them, which live in
            # the graphs' memory pool only as long as something holds them)
            self._inputs = p.stage(self.s_img, self.s_label, fg, statics)
            p.fake_pass(self._inputs, zd[0])
        first = _graph(staged_pass)
        pool = first.pool()

        def bucket_graphs(gen):
            """One graph per gradient bucket: graph k holds the launches up to the point where bucket k is final (the
            generators flag their last bucket, behind which they launch nothing more)."""
            graphs, last = [], False
            while not last:
                gk = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gk, pool=pool, capture_error_mode=_CAPTURE_MODE):
                    lo, hi, last = next(gen)
                graphs.append((gk, (lo, hi)))
            return graphs
        self.g_gf = [first] + [_graph(lambda z=z: p.fake_pass(self._inputs, z), pool) for z in zd[1:]]
        # one set of compute graphs per batch of a generator pass (each reads its own slot of the paired buffer)
        # (the apply graph of a set is captured right behind it: a fused single-rank update reads that set's raw gradients)
        self.g_dc, self.g_da = [], []
        for j in range(fg):
            self.g_dc.append(bucket_graphs(p.d_compute_iter(self._inputs, j, self._fuse_d)))
            self.g_da.append(_graph(self.d_apply, pool))
        self.g_zd = [_graph(z.normal_, pool) for z in zd]
        self.g_z = [_graph(z.normal_, pool) for z in zg]
        self.g_gc = [bucket_graphs(p.g_compute_iter(self._inputs, z)) for z in zg]
        self.g_ga = _graph(self.g_apply, pool)

    def eager_iteration(self, img, label):
        return GANTrainer.train_iteration(self, img, label)

    def train_iteration(self, img, label, zs=None):
        """Replays the captured step; `zs` (d_iters + g_iters latent batches) replaces the in-graph latent draws.  The
        paired and grouped passes are sized at capture: a batch of another shape than the captured one is refused before
        the statics are touched (the driver drops the loader's short final batch)."""
        if self._graphs is None:
            return super().train_iteration(img, label, zs)
        if tuple(img.shape) != tuple(self.s_img.shape) or tuple(label.shape) != tuple(self.s_label.shape):
            raise ValueError(f'Not valid batch: the captured step takes images {tuple(self.s_img.shape)} and labels '
                             f'{tuple(self.s_label.shape)}, got {tuple(img.shape)} and {tuple(label.shape)}; a GraphedGANTrainer '
                             'runs whole batches only (drop_last)')
        if self._hyper_key != self._hyper():
            if self.lecam is not None and self._hyper_key[-1] != self._hyper()[-1]:
                # the regulariser's numbers do not come back with a resumed optimizer state: a change is an attribute write,
                # and capturing again would change the loss mid-run without a word
                raise ValueError('Not valid LeCam regulariser: lambda, decay and start are arguments of the captured launches and '
                                 f'were {self._hyper_key[-1][1:]} at capture(), now {self.lecam.hyper()}; build a new trainer to change them')
            # betas / eps / weight decay changed since the capture (a resumed optimizer state): the apply graphs hold the
            # old values as kernel arguments -- capture again (state is snapshotted and restored around it).  The learning
            # rate is read from device memory when the kernels run: a scheduler step needs no re-capture.
            self.capture(img, label)
        self.s_img.copy_(img, non_blocking=True)
        self.s_label.copy_(label, non_blocking=True)
        if zs is not None:
            rows = self.s_zall.shape[0] // img.shape[0]            # passes * fg + g_iters (= d_iters + g_iters for today's fg)
            zs = list(zs)[:rows]
            if len(zs) < rows:
                raise ValueError(f'Not valid latents: the captured step takes {rows} latent batches, got {len(zs)}')
            self.s_zall.copy_(torch.cat(zs), non_blocking=True)
        if self.g_all is not None:
            if zs is None:
                self.g_draw.replay()
            self.g_all.replay()
            return self.loss_d, self.loss_g
        fg = self._fg
        for k in range(self.d_iters):
            if k % fg == 0:
                if zs is None:
                    self.g_zd[k // fg].replay()
                self.g_gf[k // fg].replay()
            for gk, (lo, hi) in self.g_dc[k % fg]:
                gk.replay()
                self._reduce_bucket(self.grad_d, lo, hi)
            self._join_comm()
            self.g_da[k % fg].replay()
        for i in range(self.g_iters):
            if zs is None:
                self.g_z[i].replay()
            for gk, (lo, hi) in self.g_gc[i]:
                gk.replay()
                self._reduce_bucket(self.grad_g, lo, hi)
            self._join_comm()
            self.g_ga.replay()
        return self.loss_d, self.loss_g


def batch_route(static_shapes, input_shapes) -> str:
    """Where a batch of `input_shapes` goes on a trainer whose captured statics have `static_shapes` (None: nothing is
    captured): 'replay' when every shape equals its static's, 'eager' when the inputs differ from the statics in the leading
    (batch) dimension only and agree on it among themselves (the loader's short final batch), ValueError for anything
    else -- another resolution, inputs that disagree on N, an empty batch.  A function of shapes alone: it runs before any
    copy or launch, and a copy_ into the statics would raise late (sizes that differ) or broadcast silently (N = 1)."""
    given = [tuple(int(x) for x in v) for v in input_shapes]
    if not given or any(len(v) == 0 for v in given):
        raise ValueError(f'Not valid batch: every input needs a leading batch dimension, got shapes {given}')
    ns = sorted({v[0] for v in given})
    if len(ns) != 1:
        raise ValueError(f'Not valid batch: the inputs disagree on the batch size, got shapes {given}')
    if ns[0] < 1:
        raise ValueError(f'Not valid batch: empty batch, got shapes {given}')
    if static_shapes is None:
        return 'eager'
    statics = [tuple(int(x) for x in s) for s in static_shapes]
    if len(statics) != len(given):
        raise ValueError(f'Not valid batch: the captured step takes {len(statics)} inputs, got {len(given)}')
    if given == statics:
        return 'replay'
    for s, v in zip(statics, given):
        if v[1:] != s[1:]:
            raise ValueError(f'Not valid batch: input of shape {v} differs from the captured {s} in more than the batch '
                             'dimension')
    return 'eager'


class _FlatTrainer:
    """Loop body shared by train_glow.py:108-121 and train_pixelcnn.py:108-121: zero_grad, forward, backward,
    clip_grad_norm_(parameters, 1), Adam(lr 3e-4) -- parameters and gradients each in one flat fp32 buffer, so the
    clip and the optimizer are one launch each and a data-parallel run all-reduces one bucket.  `capture` records
    forward+backward and clip+Adam as two HIP graphs; the all-reduce of a multi-rank run sits between the replays.

    Every subclass's `train_iteration` goes through `_dispatch`, which decides by shapes alone (`batch_route`): a batch that
    matches the captured statics replays; a batch of another size (the loader's short final batch, down to one sample)
    runs the eager step at its own size and leaves the graphs and their statics alone; any other mismatch raises
    ValueError before anything is copied or launched."""

    def __init__(self, model, lr=3e-4, betas=(0.9, 0.999), weight_decay=0.0, max_norm=1.0, dist_group=None, world_size=1,
                 optimizer='Adam', momentum=0.0):
        self.model = model
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.fs = FlatState(self.params)
        flat = self.fs.ensure()
        self.gflat = torch.zeros_like(flat)
        self.opt = make_fused_optimizer(optimizer, self.fs, lr, betas, momentum, weight_decay)   # train_vae.py:151-165
        self.max_norm = max_norm
        self.group, self.world = dist_group, world_size
        self.grad_norm = None
        self._graphs = None

    def _bind_grads(self):
        self.fs.ensure()
        for p, gv in zip(self.params, self.fs.views(self.gflat)):
            if p.grad is None or p.grad.data_ptr() != gv.data_ptr():
                p.grad = gv

    def _compute(self, *inputs):            # forward + backward into self.gflat; returns the loss
        raise NotImplementedError

    def _refresh(self):                     # in-graph refresh of per-step random inputs
        pass

    def _draw(self, *inputs):               # the per-step random input at the batch's own size (None: the step has none)
        return None

    def _check(self, *inputs):              # what the model refuses about a batch, before any launch
        pass

    def _dispatch(self, *inputs, rand=None):
        """One train step on `inputs` (+ `rand`, the injected per-step random tensor): replay or eager, see the class."""
        given = list(inputs) + ([rand] if rand is not None else [])
        statics = [s.shape for s in self.statics[:len(given)]] if self._graphs else None
        route = batch_route(statics, [t.shape for t in given])
        self._check(*inputs)
        if route == 'replay':
            return self._replay(*inputs, rand=rand)
        if rand is None:
            rand = self._draw(*inputs)
        return self._eager(*inputs, *(() if rand is None else (rand,)))

    def _apply(self):
        self.grad_norm = ops.clip_grad_norm_(self.gflat, self.max_norm)
        self.opt.step(self.gflat)

    def _allreduce(self):
        if self.world > 1:
            from .dist import allreduce_mean_
            allreduce_mean_(self.gflat, self.world, self.group)

    def _capture(self, statics, warmup: int):
        """`statics`: the step's inputs followed by its per-step random tensor (if the subclass has one, `_refresh`
        redraws it).  The warm-up steps run on a snapshot of model + optimizer state that is restored before the
        capture, so capturing does not advance training."""
        self.model.train(True)
        self._bind_grads()
        self.statics = statics

        def compute():
            self.loss = self._compute(*statics)

        def body():
            with torch.no_grad():
                compute()
                self._allreduce()
                self._apply()

        _rehearse(self.model, (self.opt,), body, warmup, self._bind_grads)
        with torch.no_grad():
            self.g_c = _graph(compute)
            self._has_refresh = type(self)._refresh is not _FlatTrainer._refresh
            if self._has_refresh:
                self.g_r = _graph(self._refresh, self.g_c.pool())
            self.g_a = _graph(self._apply, self.g_c.pool())
        self._graphs = True
        self._hyper_key = self.opt.hyper()

    def _replay(self, *inputs, rand=None):
        """`inputs` fill the leading statics; `rand` (optional) replaces the in-graph redraw of the last one."""
        if self._hyper_key != self.opt.hyper():
            raise RuntimeError('optimizer hyper-parameters changed after capture(): the captured optimizer launch holds the old '
                               'values -- call capture() again')
        for s, v in zip(self.statics, inputs):
            s.copy_(v, non_blocking=True)
        if self._has_refresh:
            if rand is not None:
                self.statics[-1].copy_(rand, non_blocking=True)
            else:
                self.g_r.replay()
        self.g_c.replay()
        self._allreduce()
        self.g_a.replay()
        return self.loss

    def _eager(self, *inputs):
        self.model.train(True)
        self._bind_grads()
        with torch.no_grad():
            loss = self._compute(*inputs)
            self._allreduce()
            self._apply()
        return loss


class GlowTrainer(_FlatTrainer):
    """train_glow.py:108-121 on the HIP path (see _FlatTrainer).  MCGlow or the CGlow baseline (one GPU)."""

    def __init__(self, model, *a, world_size=1, **k):
        if world_size > 1 and model._engine_cls._label_prior:
            raise ValueError('CGlow training runs on one GPU: multi-GPU CGlow is not supported; run with world_size 1')
        super().__init__(model, *a, world_size=world_size, **k)

    def _compute(self, img, label, noise):
        eng = self.model._engine()
        self.gflat.zero_()
        tape = []
        loss, _ = eng.forward(img, None, noise, True, tape, label=label)
        eng.backward(tape, img.shape[0], float(img[0].numel()))
        return loss

    def _refresh(self):
        self.statics[2].uniform_()

    def capture(self, img, label, warmup: int = 1):
        """Requires every ActNorm to be initialised already (the data-dependent init reads a device flag on the
        host, which a capture cannot do)."""
        eng = self.model._engine()
        if not eng.all_initialized():
            raise RuntimeError('GlowTrainer.capture: run the ActNorm initialisation forward first (train_glow.py:60-67)')
        eng.assume_initialized = True
        self._capture((img.clone(), label.clone(), torch.rand_like(img)), warmup)

    def _draw(self, img, label):
        return torch.rand_like(img)

    def train_iteration(self, img, label, noise=None):
        return self._dispatch(img, label, rand=noise)


class PixelCNNTrainer(_FlatTrainer):
    """train_pixelcnn.py:108-121 on the HIP path: the code map comes from the (frozen) VQ-VAE encoder upstream."""

    def __init__(self, model, *a, world_size=1, **k):
        if world_size > 1 and hasattr(model.layers[0], 'class_cond_embedding'):
            raise ValueError('CPixelCNN training runs on one GPU: multi-GPU CPixelCNN is not supported; run with world_size 1')
        super().__init__(model, *a, world_size=world_size, **k)

    def _compute(self, codes, label):
        eng = self.model._engine()
        self.gflat.zero_()
        tape = {}
        loss, _, _ = eng.forward(codes, label, True, tape, want_grad=True)
        eng.backward(tape)
        return loss

    def capture(self, codes, label, warmup: int = 1):
        self._capture((codes.clone(), label.clone()), warmup)

    def train_iteration(self, codes, label):
        return self._dispatch(codes, label)


class VAETrainer(_FlatTrainer):
    """train_vae.py:98-126 on the HIP path (config 1 of the reference runs this model on the CPU; this is the same
    loop body on the GPU kernels).  MCVAE or the CVAE baseline (one GPU).  A batch of one sample is refused, as the
    reference's BatchNorm1d refuses it in training mode (`check_train_batch`)."""

    def __init__(self, model, *a, world_size=1, **k):
        if world_size > 1 and hasattr(model.encoder, 'embedding'):
            raise ValueError('CVAE training runs on one GPU: multi-GPU CVAE is not supported; run with world_size 1')
        super().__init__(model, *a, world_size=world_size, **k)

    def _compute(self, img, label, eps):
        eng = self.model._engine()
        self.gflat.zero_()
        tape = []
        out = eng.forward(img, label, True, eps, tape, want_grad=True)
        eng.backward(tape, label)
        return out['loss']

    def _refresh(self):
        self.statics[2].normal_()

    def capture(self, img, label, warmup: int = 1):
        eps = torch.randn(img.shape[0], self.model.latent_size, device=img.device)
        self._capture((img.clone(), label.clone(), eps), warmup)

    def _draw(self, img, label):
        return torch.randn(img.shape[0], self.model.latent_size, device=img.device)

    def _check(self, img, label):
        check_train_batch(img.shape[0])

    def train_iteration(self, img, label, eps=None):
        return self._dispatch(img, label, rand=eps)


class VQVAETrainer(_FlatTrainer):
    """train_vqvae.py:99-112 on the HIP path: zero_grad, forward (the quantiser's EMA buffers move as in the reference),
    backward, clip_grad_norm_(1), Adam(lr 3e-4).  No per-step random input.  The capture warm-up restores the whole
    state_dict, the codebook buffers (embedding, cluster_size, embedding_mean) included, so capturing does not advance
    training.  A batch of another size than the captured one runs the eager step (`_FlatTrainer._dispatch`)."""

    def __init__(self, model, *a, world_size=1, **k):
        if world_size > 1:
            raise ValueError('VQVAETrainer: multi-GPU VQ-VAE training is not supported (per-rank EMA statistics would '
                             'drift the codebooks apart); run with world_size 1')
        super().__init__(model, *a, world_size=world_size, **k)

    def _compute(self, img):
        eng = self.model._engine()
        self.gflat.zero_()
        tape = []
        out = eng.forward(img, True, tape, want_grad=True)
        eng.backward(tape)
        return out['loss']

    def capture(self, img, warmup: int = 1):
        self._capture((img.clone(),), warmup)

    def train_iteration(self, img):
        return self._dispatch(img)


class ClassifierTrainer(_FlatTrainer):
    """train_classifier.py:104-113 on the HIP path: zero_grad, forward in training mode (the BatchNorm running statistics
    move as in the reference), backward, clip_grad_norm_(1), Adam (lr 1e-2 in the driver).  No per-step random input.
    The learning rate lives in device memory (FusedAdam), so a MultiStepLR step (`set_lr`) needs no re-capture.  The
    capture warm-up restores the whole state_dict, the BatchNorm buffers included, so capturing does not advance
    training.  A batch of another size than the captured one runs the eager step (`_FlatTrainer._dispatch`)."""

    def __init__(self, model, *a, world_size=1, **k):
        if world_size > 1:
            raise ValueError('ClassifierTrainer: multi-GPU classifier training is not supported (the reference wraps it in '
                             'nn.DataParallel; the datasets are small); run with world_size 1')
        super().__init__(model, *a, world_size=world_size, **k)
        self.logits = None

    def _compute(self, img, label):
        eng = self.model._engine()
        self.gflat.zero_()
        tape = []
        loss, self.logits = eng.forward(img, label, True, tape, want_grad=True)
        eng.backward(tape)
        return loss

    def set_lr(self, lr: float):
        self.opt.set_lr(lr)

    def capture(self, img, label, warmup: int = 1):
        self._capture((img.clone(), label.clone()), warmup)

    def train_iteration(self, img, label):
        return self._dispatch(img, label)
