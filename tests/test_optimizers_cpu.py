"""The optimizers of cfg['optimizer_name'] on the HIP path, the part that needs no GPU: the float64 restatements of
tests/optim_ref.py against torch.optim (the oracle of the kernel tests), FusedSGD / FusedRMSprop / FusedAdamax state in
torch.optim's state_dict format both ways, the factory, and the drivers handing the configured optimizer to the trainer."""
import os
import subprocess
import sys

import pytest
import torch

import optim_ref as OR
from test_checkpoint_compat import _small_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 0.01


def _close(got, ref, what):
    """1e-13 relative to the tensor's largest magnitude: both sides are the same double arithmetic up to the order of two
    or three operations (a few units of 2^-53 = 1.1e-16 per step, four steps)."""
    assert float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max()), what


def _torch_steps(make, grads):
    """-> [(p, state dict of the parameter)] after each step of the torch optimizer `make([p])` from p0 = grads' seed."""
    p = torch.nn.Parameter(torch.randn(1000, dtype=torch.float64, generator=torch.Generator().manual_seed(11)))
    p0 = p.detach().clone()
    opt = make([p])
    out = []
    for g in grads:
        p.grad = g.clone()
        opt.step()
        out.append((p.detach().clone(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state[p].items()}))
    return p0, out


def _grads():
    gen = torch.Generator().manual_seed(5)
    return [torch.randn(1000, dtype=torch.float64, generator=gen) for _ in range(4)]


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('mu', [0.0, 0.9])
def test_sgd_restatement_is_torch_sgd(mu, wd):
    grads = _grads()
    p, steps = _torch_steps(lambda ps: torch.optim.SGD(ps, lr=LR, momentum=mu, weight_decay=wd), grads)
    buf = torch.zeros_like(p) if mu else None
    for t, (g, (pt, st)) in enumerate(zip(grads, steps), 1):
        p, buf = OR.sgd(p, g, buf, LR, mu, wd)
        _close(p, pt, f'step {t}: p')
        if mu:
            _close(buf, st['momentum_buffer'], f'step {t}: momentum_buffer')
        else:
            assert buf is None and 'momentum_buffer' not in st


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('mu', [0.0, 0.9])
def test_rmsprop_restatement_is_torch_rmsprop(mu, wd):
    grads = _grads()
    p, steps = _torch_steps(lambda ps: torch.optim.RMSprop(ps, lr=LR, alpha=0.99, eps=1e-8, momentum=mu, weight_decay=wd), grads)
    sq, buf = torch.zeros_like(p), (torch.zeros_like(p) if mu else None)
    for t, (g, (pt, st)) in enumerate(zip(grads, steps), 1):
        p, sq, buf = OR.rmsprop(p, g, sq, buf, LR, 0.99, 1e-8, mu, wd)
        _close(p, pt, f'step {t}: p')
        _close(sq, st['square_avg'], f'step {t}: square_avg')
        if mu:
            _close(buf, st['momentum_buffer'], f'step {t}: momentum_buffer')


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_adamax_restatement_is_torch_adamax(wd):
    grads = _grads()
    p, steps = _torch_steps(lambda ps: torch.optim.Adamax(ps, lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd), grads)
    m, u = torch.zeros_like(p), torch.zeros_like(p)
    for t, (g, (pt, st)) in enumerate(zip(grads, steps), 1):
        p, m, u = OR.adamax(p, g, m, u, t, LR, 0.9, 0.999, 1e-8, wd)
        _close(p, pt, f'step {t}: p')
        _close(m, st['exp_avg'], f'step {t}: exp_avg')
        _close(u, st['exp_inf'], f'step {t}: exp_inf')


# ---- state round trip -------------------------------------------------------------------------------------------------
def _cases():
    from mcgen_amd.trainer import FusedAdamax, FusedRMSprop, FusedSGD
    return {
        'sgd': (FusedSGD, torch.optim.SGD, dict(lr=2e-4, momentum=0.9, weight_decay=0.01), ['momentum_buffer'], False),
        'rmsprop': (FusedRMSprop, torch.optim.RMSprop, dict(lr=2e-4, momentum=0.9, weight_decay=0.01),
                    ['square_avg', 'momentum_buffer'], True),
        'rmsprop0': (FusedRMSprop, torch.optim.RMSprop, dict(lr=2e-4, momentum=0.0, weight_decay=0.0), ['square_avg'], True),
        'adamax': (FusedAdamax, torch.optim.Adamax, dict(lr=2e-4, betas=(0.5, 0.999), weight_decay=0.01),
                   ['exp_avg', 'exp_inf'], True),
    }


@pytest.mark.parametrize('case', ['sgd', 'rmsprop', 'rmsprop0', 'adamax'])
def test_fused_state_is_torch_state(case):
    """state_dict() of a fused optimizer loads into the matching torch.optim class over the same parameters, and a torch
    optimizer that has taken steps loads into the fused one (the reference checkpoints optimizer.state_dict())."""
    from mcgen_amd.gan_engine import FlatState
    fused_cls, torch_cls, kw, keys, has_step = _cases()[case]
    m, _ = _small_model()
    params = list(m.generator.parameters())
    fo = fused_cls(FlatState(params), **kw)
    assert fo.state_dict()['state'] == {}                              # fresh optimizer: empty, as torch's
    g = torch.Generator().manual_seed(0)
    slots = dict(fo._slots())
    assert list(slots) == keys
    for buf in slots.values():
        buf.copy_(torch.rand(buf.shape, generator=g))
    fo.step_count.fill_(7)
    assert [t.data_ptr() for t in fo.state_tensors()] == [b.data_ptr() for b in slots.values()] + [fo.step_count.data_ptr()]
    sd = fo.state_dict()
    ref = torch_cls(params, lr=1.0)
    ref.load_state_dict(sd)                                            # torch accepts the format
    grp = ref.param_groups[0]
    for k, v in kw.items():
        assert (tuple(grp[k]) if k == 'betas' else grp[k]) == v, k
    fresh = torch_cls(params, **kw).state_dict()['param_groups'][0]
    assert set(sd['param_groups'][0]) == set(fresh)                    # the installed torch's own keys, no more, no fewer
    for p in params:
        st = ref.state[p]
        assert set(st) == set(keys) | ({'step'} if has_step else set())
        assert not has_step or int(st['step']) == 7
        for k in keys:
            assert torch.equal(st[k], fo.fs.view_of(slots[k], p)), k
    # and the other way: a torch optimizer that has taken two steps
    ref2 = torch_cls(params, **dict(kw, lr=3e-4))
    for _ in range(2):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        ref2.step()
    fb = fused_cls(FlatState(params))
    fb.load_state_dict(ref2.state_dict())
    assert fb.lr == 3e-4 and int(fb.step_count) == (2 if has_step else 1)
    for k, v in kw.items():
        if k != 'lr':
            assert getattr(fb, {'weight_decay': 'wd'}.get(k, k)) == v, k
    slots = dict(fb._slots())
    assert list(slots) == keys
    for p in params:
        for k in keys:
            assert torch.equal(fb.fs.view_of(slots[k], p), ref2.state[p][k]), k
    assert fb.hyper() == fused_cls(FlatState(params), **kw).hyper()


def _group_of(torch_cls, params, **kw):
    return torch_cls(params, lr=1e-3, **kw).state_dict()['param_groups'][0]


def test_unsupported_options_are_refused():
    """What the kernels do not implement raises 'Not valid optimizer state' instead of training with other arithmetic."""
    from mcgen_amd.gan_engine import FlatState
    from mcgen_amd.trainer import FusedAdamax, FusedRMSprop, FusedSGD
    m, _ = _small_model()
    params = list(m.generator.parameters())
    n = len(params)
    sgd, rms, amx = (cls(FlatState(params)) for cls in (FusedSGD, FusedRMSprop, FusedAdamax))
    bad = [(sgd, dict(_group_of(torch.optim.SGD, params, momentum=0.9, nesterov=True))),
           (sgd, dict(_group_of(torch.optim.SGD, params, momentum=0.9, dampening=0.1))),
           (sgd, dict(_group_of(torch.optim.SGD, params, maximize=True))),
           (rms, dict(_group_of(torch.optim.RMSprop, params, centered=True))),
           (rms, dict(_group_of(torch.optim.RMSprop, params, maximize=True))),
           (amx, dict(_group_of(torch.optim.Adamax, params, maximize=True)))]
    for opt, grp in bad:
        with pytest.raises(ValueError, match='Not valid optimizer state'):
            opt.load_state_dict({'state': {}, 'param_groups': [grp]})
    for opt, cls in ((sgd, torch.optim.SGD), (rms, torch.optim.RMSprop), (amx, torch.optim.Adamax)):
        grp = _group_of(cls, params)
        opt.load_state_dict({'state': {}, 'param_groups': [grp]})      # the plain group is fine
        with pytest.raises(ValueError, match='Not valid optimizer state'):       # more than one parameter group
            opt.load_state_dict({'state': {}, 'param_groups': [dict(grp, params=list(range(n - 1))), dict(grp, params=[n - 1])]})
    # parameters that disagree on `step`
    for opt, cls in ((rms, torch.optim.RMSprop), (amx, torch.optim.Adamax)):
        ref = cls(params, lr=1e-3)
        for p in params:
            p.grad = torch.ones_like(p)
        ref.step()
        sd = ref.state_dict()
        sd['state'][1]['step'] = torch.tensor(5.0)
        with pytest.raises(ValueError, match='Not valid optimizer state'):
            opt.load_state_dict(sd)


def test_factory_builds_the_four_optimizers():
    from mcgen_amd.gan_engine import FlatState
    from mcgen_amd.trainer import FusedAdam, FusedAdamax, FusedRMSprop, FusedSGD, make_fused_optimizer
    m, _ = _small_model()
    fs = FlatState(list(m.generator.parameters()))
    o = make_fused_optimizer('SGD', fs, 0.1, (0.5, 0.999), 0.9, 0.01)
    assert type(o) is FusedSGD and (o.lr, o.momentum, o.wd) == (0.1, 0.9, 0.01) and o.hyper() == (0.9, 0.01)
    assert o.buf is not None and make_fused_optimizer('SGD', fs, 0.1).buf is None      # no buffer without momentum
    o = make_fused_optimizer('RMSprop', fs, 0.1, (0.5, 0.999), 0.9, 0.01)
    assert type(o) is FusedRMSprop and (o.lr, o.alpha, o.eps, o.momentum, o.wd) == (0.1, 0.99, 1e-8, 0.9, 0.01)
    assert o.hyper() == (0.99, 1e-8, 0.9, 0.01) and make_fused_optimizer('RMSprop', fs, 0.1).buf is None
    o = make_fused_optimizer('Adamax', fs, 0.1, (0.5, 0.999), 0.9, 0.01)
    assert type(o) is FusedAdamax and (o.lr, o.betas, o.eps, o.wd) == (0.1, (0.5, 0.999), 1e-8, 0.01)
    assert o.hyper() == ((0.5, 0.999), 1e-8, 0.01)
    o = make_fused_optimizer('Adam', fs, 0.1, (0.5, 0.999), 0.9, 0.01)
    assert type(o) is FusedAdam and (o.lr, o.betas, o.eps, o.wd) == (0.1, (0.5, 0.999), 1e-8, 0.01)
    assert [t.data_ptr() for t in o.state_tensors()] == [o.m.data_ptr(), o.v.data_ptr(), o.step_count.data_ptr()]
    for name in ('adam', 'AdamW', '', None):
        with pytest.raises(ValueError, match='Not valid optimizer name'):
            make_fused_optimizer(name, fs, 0.1)
    d = FusedAdam(fs)                                                  # FusedAdam's own defaults stay as they were
    assert (d.lr, d.betas, d.eps, d.wd) == (2e-4, (0.5, 0.999), 1e-8, 0.0) and d.hyper() == ((0.5, 0.999), 1e-8, 0.0)
    for o in (make_fused_optimizer(n, fs, 0.1) for n in ('SGD', 'RMSprop', 'Adam', 'Adamax')):
        o.set_lr(0.05)
        assert o.lr == 0.05 and o.state_dict()['param_groups'][0]['lr'] == 0.05


_PRELUDE = r'''
import sys, os
sys.path.insert(0, os.path.join(ROOT, 'compat'))
class Stub:
    def __init__(self, model, *a, **k):
        self.a, self.k = a, k
'''
_VAE_DEFAULT = r'''
import train_vae
from config import cfg
sys.argv = ['train_vae.py', '--optimizer_name', 'Adagrad']
try:
    train_vae.parse({})
    raise SystemExit('a name outside the reference table must be refused')
except ValueError as e:
    assert str(e) == 'Not valid optimizer name'
sys.argv = ['train_vae.py', '--data_name', 'CIFAR10', '--model_name', 'mcvae']
extra = train_vae.parse({'pivot_metric': 'BCE'})
assert extra['engine'] == 'fused' and cfg['optimizer_name'] == 'Adam' and cfg['momentum'] == 0
drv = train_vae.VAEDriver(extra)
drv.trainer_cls = Stub
k = drv.make_trainer(object()).k
assert (k['optimizer'], k['momentum'], k['weight_decay'], k['lr'], k['world_size']) == ('Adam', 0, 0, 3e-4, 1), k
'''
_VAE_FLAGS = r'''
import train_vae
from config import cfg
sys.argv = ['train_vae.py', '--data_name', 'CIFAR10', '--optimizer_name', 'RMSprop', '--model_name', 'mcvae', '--momentum=0.9']
extra = train_vae.parse({'pivot_metric': 'BCE'})
assert cfg['optimizer_name'] == 'RMSprop' and cfg['momentum'] == 0.9 and cfg['model_name'] == 'mcvae'
cfg['weight_decay'] = 0.01
drv = train_vae.VAEDriver(extra)
drv.trainer_cls = Stub
k = drv.make_trainer(object()).k
assert (k['optimizer'], k['momentum'], k['weight_decay'], k['lr']) == ('RMSprop', 0.9, 0.01, 3e-4), k
'''
_GAN_FLAGS = r'''
import mcgen_amd.trainer
mcgen_amd.trainer.GraphedGANTrainer = Stub
import train_gan
from config import cfg
sys.argv = ['train_gan.py', '--data_name', 'CIFAR10', '--model_name', 'mcgan', '--optimizer_name', 'SGD', '--momentum', '0.5']
train_gan.parse()
cfg['classes_size'], cfg['weight_decay'] = 10, 0.02
tr = train_gan.make_trainer(object(), 2e-4, (0.5, 0.999))
assert tr.a == (10,) and (tr.k['optimizer'], tr.k['momentum'], tr.k['weight_decay'], tr.k['lr'], tr.k['betas']) == \
    ('SGD', 0.5, 0.02, 2e-4, (0.5, 0.999)), (tr.a, tr.k)
# --engine autograd: the reference's four branches (train_gan.py:222-236)
import torch
lin = torch.nn.Linear(2, 2)
cfg['momentum'] = 0.9
for name, cls in (('SGD', torch.optim.SGD), ('RMSprop', torch.optim.RMSprop), ('Adam', torch.optim.Adam), ('Adamax', torch.optim.Adamax)):
    cfg['optimizer_name'] = name
    o = train_gan.make_optimizer(lin, 2e-4, (0.5, 0.999))
    g = o.param_groups[0]
    assert type(o) is cls and g['lr'] == 2e-4 and g['weight_decay'] == 0.02
    assert g.get('momentum', 0.9) == 0.9 and tuple(g.get('betas', (0.5, 0.999))) == (0.5, 0.999)
cfg['optimizer_name'] = 'Adagrad'
try:
    train_gan.make_optimizer(lin, 2e-4, (0.5, 0.999))
    raise SystemExit('a name outside the reference table must be refused')
except ValueError as e:
    assert str(e) == 'Not valid optimizer name'
'''
_GAN_DEFAULT = r'''
import mcgen_amd.trainer
mcgen_amd.trainer.GraphedGANTrainer = Stub
import train_gan
from config import cfg
sys.argv = ['train_gan.py', '--data_name', 'CIFAR10', '--model_name', 'mcgan']
train_gan.parse()
cfg['classes_size'] = 10
k = train_gan.make_trainer(object(), 2e-4, (0.5, 0.999)).k
assert (k['optimizer'], k['momentum'], k['weight_decay']) == ('Adam', 0, 0), k
'''


@pytest.mark.parametrize('body', [_VAE_DEFAULT, _VAE_FLAGS, _GAN_FLAGS, _GAN_DEFAULT], ids=['vae', 'vae-flags', 'gan-flags', 'gan'])
def test_drivers_hand_the_configured_optimizer_to_the_trainer(body):
    """--optimizer_name / --momentum reach cfg past the drivers' hard `optimizer_name = 'Adam'`, and the fused branch of
    both drivers builds its trainer with cfg's optimizer, momentum and weight decay (a stub stands in for the trainer
    class: nothing here touches the GPU); without the flags the trainer gets Adam, as before.  One process per case:
    a driver parses its command line once."""
    code = (_PRELUDE + body + "print('WIRING-OK')\n").replace('ROOT', repr(ROOT))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'WIRING-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
