"""The averaged generator without a GPU: flag parsing, the (de)serialised layout of trainer.FusedEMA, the overlay that
--use_ema loads, and the checkpoint's keys with averaging off."""
import os
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location('_ema_flags_under_test', os.path.join(ROOT, 'compat', '_flags.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Gen(nn.Module):
    """The kinds of entries a generator's state_dict has: weights, BatchNorm (affine, running statistics, the int64
    counter) and a codebook buffer."""

    def __init__(self):
        super().__init__()
        self.linear = nn.Linear(5, 7)
        self.bn = nn.BatchNorm2d(3)
        self.conv = nn.Conv2d(3, 2, 3)
        self.register_buffer('codebook', torch.randint(0, 2, (4, 3)).float())


def test_flag_defaults_and_values():
    f = _flags()
    argv = ['train_gan.py', '--data_name', 'CIFAR10']
    assert f.pop_ema_flags(argv) == {'ema_decay': 0.0, 'ema_start': 0}
    assert f.pop_use_ema(argv) is False
    assert argv == ['train_gan.py', '--data_name', 'CIFAR10']
    argv = ['x', '--ema_decay', '0.999', '--num_epochs', '2', '--ema_start=40', '--use_ema', 'True']
    assert f.pop_ema_flags(argv) == {'ema_decay': 0.999, 'ema_start': 40}
    assert f.pop_use_ema(argv) is True
    assert argv == ['x', '--num_epochs', '2']
    for bad in (['x', '--ema_decay', '1.0'], ['x', '--ema_decay', '-0.1'], ['x', '--ema_start', '-1']):
        with pytest.raises(ValueError):
            f.pop_ema_flags(bad)
    with pytest.raises(ValueError):
        f.pop_use_ema(['x', '--use_ema', 'yes'])
    f.check_use_ema(True, 'mcgan'); f.check_use_ema(True, 'cgan'); f.check_use_ema(False, 'mcvae')
    with pytest.raises(ValueError):
        f.check_use_ema(True, 'mcvae')


def test_state_dict_layout_from_fabricated_dict():
    """FusedEMA on CPU tensors: names as in generator.state_dict(), fp32 tensors of the parameters' shapes, 'step' an int
    that survives the round trip; load_state_dict refuses other names and shapes."""
    from mcgen_amd.gan_engine import FlatState
    from mcgen_amd.trainer import FusedEMA, ema_buffers
    torch.manual_seed(0)
    gen = _Gen()
    names = [k for k, _ in gen.named_parameters()]
    bufs = ema_buffers(gen)
    assert list(bufs) == ['bn.running_mean', 'bn.running_var']            # not the codebook, not num_batches_tracked
    ema = FusedEMA(FlatState(list(gen.parameters())), bufs, 0.9, 3, names=names)
    assert ema.hyper() == (0.9, 3)
    sd = ema.state_dict()
    assert set(sd) == {'decay', 'start', 'step', 'params', 'buffers'}
    assert (sd['decay'], sd['start'], sd['step']) == (0.9, 3, 0) and type(sd['step']) is int
    gsd = gen.state_dict()
    assert list(sd['params']) == names and list(sd['buffers']) == list(bufs)
    for k, v in list(sd['params'].items()) + list(sd['buffers'].items()):
        assert v.dtype == torch.float32 and v.shape == gsd[k].shape and torch.equal(v, gsd[k]), k   # starts as the parameters
    # a fabricated dict of the same layout goes in and comes back out
    fab = {'decay': 0.5, 'start': 1, 'step': 17,
           'params': {k: torch.full_like(v, i + 1.0) for i, (k, v) in enumerate(sd['params'].items())},
           'buffers': {k: torch.full_like(v, -(i + 1.0)) for i, (k, v) in enumerate(sd['buffers'].items())}}
    ema.load_state_dict(fab)
    back = ema.state_dict()
    assert (back['decay'], back['start'], back['step']) == (0.5, 1, 17) and ema.hyper() == (0.5, 1)
    for kind in ('params', 'buffers'):
        for k, v in fab[kind].items():
            assert torch.equal(back[kind][k], v), k
    for k, v in gen.state_dict().items():                                # the live network did not move
        assert torch.equal(v, gsd[k]), k
    assert len(ema.state_tensors()) == 3 and ema.state_tensors()[-1].dtype == torch.int64
    wrong = dict(fab, params=dict(list(fab['params'].items())[1:]))
    with pytest.raises(ValueError):
        ema.load_state_dict(wrong)
    wrong = dict(fab, buffers={k: v[:-1] for k, v in fab['buffers'].items()})
    with pytest.raises(ValueError):
        ema.load_state_dict(wrong)
    with pytest.raises(ValueError):
        FusedEMA(FlatState(list(_Gen().parameters())), {}, 1.0)


def test_overlay_replaces_params_and_statistics_only():
    from mcgen_amd.checkpoint import overlay_averaged_generator
    torch.manual_seed(1)
    gen = _Gen()
    gen.bn.num_batches_tracked.fill_(5)
    gsd = {k: v.clone() for k, v in gen.state_dict().items()}
    ema = {'decay': 0.9, 'start': 0, 'step': 4,
           'params': {k: torch.randn_like(v) for k, v in gen.named_parameters()},
           'buffers': {'bn.running_mean': torch.randn(3), 'bn.running_var': torch.rand(3) + 0.5}}
    out = overlay_averaged_generator(gen.state_dict(), {'model_dict': {}, 'generator_ema': ema})
    assert list(out) == list(gsd)
    for k in gsd:
        if k in ema['params'] or k in ema['buffers']:
            want = ema['params'].get(k, ema['buffers'].get(k))
            assert torch.equal(out[k], want) and not torch.equal(out[k], gsd[k]), k
        else:
            assert k in ('codebook', 'bn.num_batches_tracked') and torch.equal(out[k], gsd[k]), k
    gen.load_state_dict(out)                                              # and it loads strictly
    assert int(gen.bn.num_batches_tracked) == 5
    with pytest.raises(ValueError, match=r'Not valid checkpoint: no averaged generator \(train with --ema_decay\)'):
        overlay_averaged_generator(gen.state_dict(), {'model_dict': {}})
    bad = dict(ema, params=dict(ema['params'], extra=torch.zeros(1)))
    with pytest.raises(ValueError):
        overlay_averaged_generator(gen.state_dict(), {'generator_ema': bad})


class _Opt:
    def state_dict(self):
        return {'state': {}, 'param_groups': []}


def test_checkpoint_keys_with_averaging_off_and_on():
    from mcgen_amd.checkpoint import make_checkpoint
    from mcgen_amd.gan_engine import FlatState
    from mcgen_amd.trainer import FusedEMA, ema_buffers
    gen = _Gen()
    opt = {'generator': _Opt(), 'discriminator': _Opt()}
    today = {'cfg', 'epoch', 'model_dict', 'optimizer_dict', 'scheduler_dict', 'logger'}
    assert set(make_checkpoint(gen, opt, 2, {'a': 1})) == today
    assert set(make_checkpoint(gen, opt, 2, {'a': 1}, ema=None)) == today
    ema = FusedEMA(FlatState(list(gen.parameters())), ema_buffers(gen), 0.9, 0, names=[k for k, _ in gen.named_parameters()])
    ck = make_checkpoint(gen, opt, 2, {'a': 1}, ema=ema)
    assert set(ck) == today | {'generator_ema'}
    assert set(ck['generator_ema']) == {'decay', 'start', 'step', 'params', 'buffers'}
    assert all(not v.is_cuda for v in ck['generator_ema']['params'].values())
