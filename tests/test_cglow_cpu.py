"""CGlow (models/cglow.py): module surface, reference checkpoints, the library surface, the trainer's and the train_glow
driver's model-name / control handling, and the float64 restatement of the label-conditioned prior against autograd.
CPU only."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cglow_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def glow_cfg():
    from mcgen_amd.config import cfg
    saved = {k: v for k, v in cfg.items()}

    def set_(classes, channels):
        cfg.update(model_name='cglow', device='cpu', classes_size=classes, data_shape=[channels, 32, 32])
        cfg['glow'] = dict(R.GLOW_CFG)
        return cfg
    yield set_
    cfg.clear()
    cfg.update(saved)


@pytest.mark.parametrize('fixture,classes,channels', R.FIXTURES)
def test_state_dict_layout_and_strict_load(glow_cfg, fixture, classes, channels):
    from mcgen_amd import models
    d = R.load(fixture)
    shapes = R.layout(d)
    glow_cfg(classes, channels)
    np.random.seed(0)
    m = models.cglow()
    own = m.state_dict()
    assert list(own) == list(shapes) and len(shapes) == 162
    assert {k: tuple(v.shape) for k, v in own.items()} == shapes
    sd0, init, final = R.states(d)
    for k, v in sd0.items():
        assert own[k].dtype == v.dtype, k
    for k in ('blocks.0.flows.0.coupling.net.0.weight', 'blocks.0.flows.1.coupling.net.6.scale', 'blocks.2.flows.1.coupling.net.4.loc',
              'blocks.0.embedding.scale', 'blocks.1.embedding.conv.weight', 'blocks.2.embedding.conv.bias', 'blocks.2.prior.conv.weight'):
        assert k in shapes, k
    assert not any('module' in k or 'codebook' in k for k in shapes)
    c = channels
    for i in range(3):                                       # every block owns an embedding over 8 x its input channels
        assert shapes[f'blocks.{i}.embedding.conv.weight'] == (8 * c, classes, 1, 1)
        c *= 2
    for sd in (sd0, init, final):
        m.load_state_dict(sd, strict=True)
    assert [tuple(s) for s in m.make_z_shapes()] == [(2 * channels, 16, 16), (4 * channels, 8, 8), (16 * channels, 4, 4)]


def test_fixture_labels_and_perturbation():
    """What the fixtures have to exercise: a repeated label, the last mode, most modes absent; non-zero ZeroConv2d scales."""
    for fixture, classes, _ in R.FIXTURES:
        d = R.load(fixture)
        lab = d['label']
        assert len(set(lab.tolist())) < len(lab) and classes - 1 in lab and len(set(lab.tolist())) < classes / 2
        for k in ('blocks.2.embedding.scale', 'blocks.2.prior.scale', 'blocks.2.embedding.conv.weight', 'blocks.0.embedding.conv.bias'):
            assert float(np.abs(d['sd/' + k]).min()) > 0, k
        assert not any(k.startswith('grad0/blocks.0.embedding') or k.startswith('grad0/blocks.1.embedding') for k in d)
        assert float(np.abs(d['grad0/blocks.2.prior.conv.weight']).max()) == 0.0
        absent = sorted(set(range(classes)) - set(lab.tolist()))
        assert float(np.abs(d['grad0/blocks.2.embedding.conv.weight'][:, absent]).max()) == 0.0
        assert float(np.abs(d['grad0/blocks.2.embedding.scale']).max()) > 0


def test_constructor_refuses_unbuilt_forms(glow_cfg):
    from mcgen_amd import models
    cfg = glow_cfg(12, 1)
    for key in ('affine', 'conv_lu'):
        cfg['glow'] = dict(R.GLOW_CFG, **{key: False})
        with pytest.raises(ValueError):
            models.cglow()


def test_exports():
    from mcgen_amd import models
    from mcgen_amd.glow_engine import CGlowEngine, GlowEngine
    assert models.cglow and models.CGlow and issubclass(CGlowEngine, GlowEngine) and models.CGlow._engine_cls is CGlowEngine
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        import importlib
        cm = importlib.import_module('models')
        assert cm.cglow is models.cglow and cm.CGlow is models.CGlow
        assert 'cglow.py' in cm.__doc__ and 'cvae.py' in cm.__doc__ and '(cvae, cglow)' not in cm.__doc__
        assert "stays the reference's own file" not in cm.__doc__
    finally:
        sys.path.remove(os.path.join(ROOT, 'compat'))


def test_library_exports_cglow_kernels():
    from mcgen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.mcgen_abi_version() == 9
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mcgen_cglow_prior', 'mcgen_cglow_prior_bwd'):
        assert hasattr(raw, name) and name in _lib.SYMBOLS and name in _lib.HEADER.functions, name
    assert 'cglow_ops' in open(os.path.join(ROOT, 'multimodal-controller-for-generative-models_amd', 'csrc', 'build.sh')).read()
    # host-side argument checks, before any launch
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    fwd, bwd = lib.mcgen_cglow_prior, lib.mcgen_cglow_prior_bwd
    assert fwd(None, None, None, None, None, None, None, 0, 4, 16, 32, 12, 32, None) != 0
    assert b'cglow_prior' in lib.mcgen_last_error()
    assert fwd(p, p, p, p, p, p, p, 0, 4, 16, 32, 12, 24, None) != 0                     # Cp below C2
    assert fwd(p, p, p, p, p, p, p, 0, 4, 16, 32, 12, 36, None) != 0                     # Cp no multiple of 8
    assert fwd(p, p, p, p, p, p, p, 0, 4, 16, 31, 12, 32, None) != 0                     # odd channel count
    assert fwd(p, p, p, p, p, p, p, 0, 4, 16, 32, 0, 32, None) != 0                      # no modes
    assert fwd(p, p, p, p, p, p, p, 0, 0, 16, 32, 12, 32, None) != 0                     # no samples
    assert fwd(p, p, p, p, p, p, p, 0, 4, 16, 16384, 12, 16384, None) != 0               # beyond the LDS row
    assert b'cglow_prior' in lib.mcgen_last_error()
    assert fwd(p, p, p, p, p, p, p, 7, 4, 16, 32, 12, 32, None) != 0                     # no such dtype
    assert b'cglow_prior' in lib.mcgen_last_error()
    assert bwd(None, None, None, None, None, None, None, None, None, None, None, 0, None, None, None, 0, 4, 16, 32, 12, 32, None) != 0
    assert b'cglow_prior_bwd' in lib.mcgen_last_error()
    assert bwd(p, p, p, p, p, p, p, p, p, p, None, 0, p, p, p, 0, 4, 16, 32, 12, 24, None) != 0           # Cp below C2
    assert bwd(p, p, p, p, p, p, p, None, p, p, None, 0, p, p, p, 0, 4, 16, 32, 12, 32, None) != 0        # no workspace
    assert bwd(p, p, p, p, p, p, p, p, p, p, p, 0, p, p, p, 0, 4, 16, 32, 12, 32, None) != 0              # dw_p without its size
    assert bwd(p, p, p, p, p, p, p, p, p, p, None, 9, p, p, p, 0, 4, 16, 32, 12, 32, None) != 0           # a size without dw_p
    assert bwd(p, p, p, p, p, p, p, p, p, p, None, 0, p, p, p, 7, 4, 16, 32, 12, 32, None) != 0           # no such dtype
    assert b'cglow_prior_bwd' in lib.mcgen_last_error()


def test_forward_has_no_cpu_fallback(glow_cfg):
    from mcgen_amd import _lib, models
    glow_cfg(12, 1)
    m = models.cglow()
    inp = {'img': torch.zeros(2, 1, 32, 32), 'label': torch.zeros(2, dtype=torch.long)}
    for train in (True, False):
        m.train(train)
        with pytest.raises((_lib.McgenError, RuntimeError, NotImplementedError)):
            m(inp)
    with pytest.raises((_lib.McgenError, RuntimeError, NotImplementedError)):
        m.generate(inp['label'])


def test_bad_labels_raise(glow_cfg):
    from mcgen_amd import models
    glow_cfg(12, 1)
    m = models.cglow()
    img = torch.zeros(1, 1, 32, 32)
    for bad in (torch.tensor([12]), torch.tensor([-1]), torch.tensor([1], dtype=torch.int32), torch.tensor([[1]])):
        with pytest.raises(ValueError):
            m({'img': img, 'label': bad})
        with pytest.raises(ValueError):
            m.generate(bad)


def test_trainer_refuses_multi_gpu(glow_cfg):
    from mcgen_amd import models
    from mcgen_amd.trainer import GlowTrainer
    glow_cfg(12, 1)
    with pytest.raises(ValueError, match='one GPU'):
        GlowTrainer(models.cglow(), world_size=2)


@pytest.mark.parametrize('modes,c2,hw', [(10, 96, 16), (1623, 32, 16), (12, 8, 4)])
def test_float64_restatement_matches_autograd(modes, c2, hw):
    """The formulas of cglow_ref against autograd through the reference's own expression: two ZeroConv2d modules written with
    F.conv2d, the 3x3 one on zeros, the 1x1 one on the one-hot label broadcast over the pixels."""
    g = torch.Generator().manual_seed(modes)
    n, side, c = 9, int(hw ** 0.5), c2 // 2
    f64 = torch.float64
    w_p = torch.randn(c2, c, 3, 3, generator=g, dtype=f64).requires_grad_(True)
    b_p, s_p, b_e, s_e = ((0.3 * torch.randn(c2, generator=g, dtype=f64)).requires_grad_(True) for _ in range(4))
    w_e = (0.3 * torch.randn(c2, modes, 1, 1, generator=g, dtype=f64)).requires_grad_(True)
    label = torch.randint(0, modes, (n,), generator=g)
    label[0] = modes - 1; label[1] = label[2]
    dprior = torch.randn(n, c2, side, side, generator=g, dtype=f64)
    zero = torch.zeros(n, c, side, side, dtype=f64)
    h = F.conv2d(zero, w_p, b_p, 1, 1) * torch.exp(s_p.view(1, -1, 1, 1) * 3)
    ind = F.one_hot(label, modes).to(f64)
    h = h + F.conv2d(ind.view(n, modes, 1, 1), w_e, b_e) * torch.exp(s_e.view(1, -1, 1, 1) * 3)
    (h * dprior).sum().backward()
    args = [t.detach().numpy() for t in (b_p, s_p, w_e.view(c2, modes), b_e, s_e)]
    got = R.prior(*args, label.numpy(), hw)
    assert np.abs(got - h.detach().permute(0, 2, 3, 1).reshape(n, hw, c2).numpy()).max() < 1e-12
    grads = R.prior_bwd(dprior.permute(0, 2, 3, 1).reshape(n, hw, c2).numpy(), *args, label.numpy())
    ref = {'b_p': b_p.grad, 's_p': s_p.grad, 'w_e': w_e.grad.view(c2, modes), 'b_e': b_e.grad, 's_e': s_e.grad}
    for k, v in ref.items():
        assert np.abs(grads[k] - v.numpy()).max() < 1e-10 * max(1.0, float(v.abs().max())), k
    assert float(w_p.grad.abs().max()) == 0.0
    absent = sorted(set(range(modes)) - set(label.tolist()))
    assert float(np.abs(grads['w_e'][:, absent]).max()) == 0.0
    # a label outside the table: a zero embedding row, no table gradient
    lab2 = label.numpy().copy(); lab2[3] = modes; lab2[4] = -1
    h2 = R.prior(*args, lab2, hw)
    assert np.abs(h2[3, 0] - (args[0] * np.exp(3 * args[1]) + args[3] * np.exp(3 * args[4]))).max() < 1e-12
    ok = np.array([i not in (3, 4) for i in range(n)])
    g2 = R.prior_bwd(dprior.permute(0, 2, 3, 1).reshape(n, hw, c2).numpy(), *args, lab2)
    g3 = R.prior_bwd(dprior.permute(0, 2, 3, 1).reshape(n, hw, c2).numpy()[ok], *args, lab2[ok])
    assert np.abs(g2['w_e'] - g3['w_e']).max() < 1e-12


_PROBE = r'''
import json, sys
sys.path.insert(0, {compat!r})
sys.argv = ['train_glow.py'] + {args!r}
import train_glow as T
import _single
captured = {{}}
def fake_main(self):
    from utils import process_control
    process_control()
    cfg = _single.cfg
    tag = [str(cfg['init_seed']), cfg['data_name'], cfg['subset'], cfg['model_name'], cfg['control_name']]
    captured.update(tag='_'.join(x for x in tag if x), control=cfg['control'], glow=cfg['glow'])
T.GlowDriver.main = fake_main
try:
    T.main()
except ValueError as e:
    captured['error'] = str(e)
print(json.dumps(captured))
'''


def _probe(args, tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    code = _PROBE.format(compat=os.path.join(ROOT, 'compat'), args=args)
    r = subprocess.run([sys.executable, '-c', code], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_train_glow_cglow_tag(tmp_path):
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'cglow', '--control_name', 'None'], tmp_path)
    assert c['tag'] == '0_CIFAR10_label_cglow' and c['control'] == {}
    assert c['glow'] == {'hidden_size': 512, 'K': 16, 'L': 3, 'affine': True, 'conv_lu': True}
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'cglow', '--control_name', 'None', '--world_size', '2'], tmp_path)
    assert 'one GPU' in c['error']


def test_train_glow_keeps_mc_tags_and_refuses_other_models(tmp_path):
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'mcglow', '--control_name', '0.5'], tmp_path)
    assert c['tag'] == '0_CIFAR10_label_mcglow_0.5' and c['control'] == {'controller_rate': '0.5'}
    for other in ('mcvae', 'cvae', 'mcgan'):
        c = _probe(['--data_name', 'CIFAR10', '--model_name', other, '--control_name', 'None'], tmp_path)
        assert c == {'error': 'Not valid model name'}
