"""CPU-side checks of the classifier training surface (no GPU): the reference fixture's loop body against an fp64
torch.nn.functional restatement of train_classifier.py:104-113 (conv, batch_norm(training=True), relu, max_pool2d,
linear, cross-entropy, clip_grad_norm_(1), Adam(1e-2)), the library exports, the driver's parsed configuration and its
refusals."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = {'coil100': ([3, 32, 32], 100, 7411), 'gray': ([1, 32, 32], 16, 7412)}       # tools/gen_golden.py CLASSIFIER_SMALL
STAGES = (0, 4, 8, 12)                                                              # Conv2d indices in `blocks`
CONV_BIASES = tuple(f'blocks.{i}.bias' for i in STAGES)


def _initial_state(shape, classes, seed):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name='classifier', device='cpu', classes_size=classes, data_shape=list(shape), compute_dtype='float32')
    cfg['classifier'] = {'hidden_size': [8, 16, 32, 64]}
    shapes = {k: tuple(v.shape) for k, v in models.classifier().state_dict().items()}
    return gu.procedural_state_generic(shapes, seed=seed)


def _forward(p, buf, img, label):
    """classifier.py:14-52 in training mode, fp64; `buf` running statistics are updated in place (momentum 0.1)."""
    x = img
    for s, i in enumerate(STAGES):
        x = F.conv2d(x, p[f'blocks.{i}.weight'], p[f'blocks.{i}.bias'], padding=1)
        x = F.batch_norm(x, buf[f'blocks.{i + 1}.running_mean'], buf[f'blocks.{i + 1}.running_var'], p[f'blocks.{i + 1}.weight'],
                         p[f'blocks.{i + 1}.bias'], training=True, momentum=0.1, eps=1e-5)
        x = F.relu(x)
        if s < len(STAGES) - 1:
            x = F.max_pool2d(x, 2)
    logits = F.linear(x.flatten(1), p['classifier.weight'], p['classifier.bias'])
    return F.cross_entropy(logits, label), logits


def _train_fp64(sd, img, label, steps, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0):
    p = {k: v.double().clone().requires_grad_(True) for k, v in sd.items() if not k.endswith(('running_mean', 'running_var',
                                                                                                 'num_batches_tracked'))}
    buf = {k: v.double().clone() for k, v in sd.items() if k.endswith(('running_mean', 'running_var'))}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    losses, logits, grads = [], [], None
    for t in range(1, steps + 1):
        for q in p.values():
            q.grad = None
        loss, lg = _forward(p, buf, img.double(), label)
        loss.backward()
        if t == 1:
            grads = {k: q.grad.clone() for k, q in p.items()}
        with torch.no_grad():
            norm = torch.sqrt(sum((q.grad ** 2).sum() for q in p.values()))
            coef = max_norm / (norm + 1e-6)
            for k, q in p.items():
                g = q.grad * coef if coef < 1 else q.grad
                m[k].mul_(betas[0]).add_(g, alpha=1 - betas[0])
                v2[k].mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
                denom = (v2[k] / (1 - betas[1] ** t)).sqrt() + eps
                q.sub_(lr / (1 - betas[0] ** t) * m[k] / denom)
        losses.append(float(loss.detach())); logits.append(lg.detach())
    return losses, logits, grads, {**{k: q.detach() for k, q in p.items()}, **buf}


@pytest.mark.parametrize('tag', ['coil100', 'gray'])
def test_fixture_matches_fp64_restatement(tag):
    d = gu.load_npz('classifier_train_small.npz')
    shape, classes, seed = SMALL[tag]
    sd = _initial_state(shape, classes, seed)
    img, label = gu.synthetic_batch(16, classes, seed=int(d[f'{tag}/input_seed']), shape=tuple(shape))
    losses, logits, grads, final = _train_fp64(sd, img, label, 3)
    assert abs(losses[0] - d[f'{tag}/losses'][0]) < 1e-6 * abs(losses[0])
    ref = torch.from_numpy(d[f'{tag}/logits'][0]).double()
    assert float((logits[0] - ref).abs().max()) < 1e-5 * float(ref.abs().max())
    for k, g in grads.items():
        r = torch.from_numpy(d[f'{tag}/grad1/{k}']).double()
        if k in CONV_BIASES:            # before a training-mode BatchNorm: 0 in exact arithmetic, rounding noise in fp32
            assert float(g.abs().max()) < 1e-12 and float(r.abs().max()) < 1e-5, k
        else:
            assert float((g - r).abs().max()) < 1e-5 * float(g.abs().max()), k
    # the later steps: the fp32 reference's conv-bias noise becomes +-lr Adam steps; the rest tracks the fp64 restatement
    np.testing.assert_allclose(losses, d[f'{tag}/losses'], rtol=1e-3)
    for k, v in final.items():
        r = torch.from_numpy(d[f'{tag}/sd_final/{k}']).double()
        if k == 'classifier.weight':
            v = v[::4]
        diff = (v - r).abs()
        if k in CONV_BIASES:
            assert float(diff.max()) < 0.1, k
        elif k.endswith('running_mean'):
            assert float(diff.max()) < 0.03 + 1e-4, k
        else:
            assert float((diff > 1e-4).double().mean()) < 2e-3 and float(diff.max()) < 2e-2, (k, float(diff.max()))
    assert all(int(d[f'{tag}/sd_final/blocks.{i + 1}.num_batches_tracked']) == 3 for i in STAGES)


def test_library_exports_maxpool_bn_backward():
    from mcgen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in ('mcgen_maxpool2_bn_bwd_stats', 'mcgen_maxpool2_bn_bwd_apply'):
        assert hasattr(raw, name) and name in _lib.SYMBOLS and name in _lib.HEADER.functions, name
        assert re.search(rf' T {name}$', nm, re.M), name
    # host-side argument checks, before any launch
    assert lib.mcgen_maxpool2_bn_bwd_stats(None, None, None, None, None, None, None, 1, 0, 1, 1, 1, 8, None) != 0
    assert b'maxpool2_bn_bwd_stats' in lib.mcgen_last_error()
    assert lib.mcgen_maxpool2_bn_bwd_apply(None, None, None, None, None, None, None, None, 0, 1, 1, 1, 8, None) != 0


def test_training_forward_has_no_cpu_fallback():
    from mcgen_amd import _lib, models
    _initial_state([3, 32, 32], 100, 1)
    m = models.classifier()
    m.train(True)
    with pytest.raises(_lib.McgenError):
        m({'img': torch.zeros(2, 3, 32, 32), 'label': torch.zeros(2, dtype=torch.long)})
    with pytest.raises(_lib.McgenError):                                  # feature() stays evaluation-only
        m.feature({'img': torch.zeros(2, 3, 32, 32)})


_PROBE = r'''
import json, sys
sys.path.insert(0, {compat!r})
sys.argv = ['train_classifier.py'] + {args!r}
import train_classifier as T
from config import cfg
T.configure()
tag = '_'.join(x for x in ['0', cfg['data_name'], cfg['subset'], cfg['model_name'], cfg['control_name']] if x)
print(json.dumps(dict(tag=tag, lr=cfg['lr'], wd=cfg['weight_decay'], sched=cfg['scheduler_name'], milestones=cfg['milestones'],
                      factor=cfg['factor'], epochs=cfg['num_epochs'], pivot=cfg['pivot'], pivot_metric=cfg['pivot_metric'],
                      metrics=cfg['metric_name'], optimizer=cfg['optimizer_name'],
                      pivot_max=T.ClassifierDriver.pivot_max)))
'''


def _probe(args, tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    code = _PROBE.format(compat=os.path.join(ROOT, 'compat'), args=args)
    return subprocess.run([sys.executable, '-c', code], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)


def test_train_classifier_parsed_config(tmp_path):
    r = _probe(['--data_name', 'COIL100', '--model_name', 'classifier', '--control_name', 'None'], tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    c = json.loads(r.stdout.strip().splitlines()[-1])
    assert c['tag'] == '0_COIL100_label_classifier'
    assert c['lr'] == 1e-2 and c['wd'] == 0 and c['optimizer'] == 'Adam'
    assert c['sched'] == 'MultiStepLR' and c['milestones'] == [100] and c['factor'] == 0.1
    assert c['epochs'] == 200
    assert c['pivot_metric'] == 'Accuracy' and c['pivot'] == -float('inf')          # maximised
    assert c['metrics'] == {'train': ['Loss', 'Accuracy'], 'test': ['Loss', 'Accuracy']}
    assert c['pivot_max'] is True


def test_train_classifier_driver_refuses_world_size_and_other_models(tmp_path):
    drv = os.path.join(ROOT, 'compat', 'train_classifier.py')
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, drv, '--data_name', 'COIL100', '--model_name', 'classifier', '--control_name', 'None',
                        '--world_size', '2'], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'world_size' in r.stderr
    r = subprocess.run([sys.executable, drv, '--data_name', 'COIL100', '--model_name', 'mcgan', '--control_name', 'None'],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'Not valid model name' in r.stderr
