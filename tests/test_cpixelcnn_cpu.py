"""CPixelCNN (models/cpixelcnn.py): module surface, parameter counts, reference checkpoints, the library surface and the
train_pixelcnn driver's model-name / control handling.  CPU only."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def px_cfg():
    from mcgen_amd.config import cfg
    saved = {k: v for k, v in cfg.items()}

    def set_(hidden, layers, codes, classes):
        cfg.update(model_name='cpixelcnn', device='cpu', classes_size=classes)
        cfg['pixelcnn'] = {'num_layer': layers, 'hidden_size': hidden, 'num_embedding': codes}
        return cfg
    yield set_
    cfg.clear()
    cfg.update(saved)


def layout(d):
    """The reference's state_dict layout a fixture recorded: {key: shape}, in state_dict order."""
    out = {}
    for s in d['layout']:
        k, dims = str(s).rsplit(':', 1)
        out[k] = tuple(int(x) for x in dims.split('x')) if dims else ()
    return out


@pytest.mark.parametrize('classes,total', [(10, 6406016), (100, 6751616), (1623, 12599936)])
def test_parameter_counts(px_cfg, classes, total):
    from mcgen_amd import models
    px_cfg(128, 15, 512, classes)
    m = models.cpixelcnn()
    assert sum(p.numel() for p in m.parameters()) == total
    assert tuple(m.layers[3].class_cond_embedding.weight.shape) == (classes, 256)


@pytest.mark.parametrize('fixture,classes', [('cpixelcnn_small.npz', 10), ('cpixelcnn_omniglot_small.npz', 1623),
                                             ('cpixelcnn_full_digest.npz', 10)])
def test_state_dict_layout_and_strict_load(px_cfg, fixture, classes):
    from mcgen_amd import models
    d = gu.load_npz(fixture)
    shapes = layout(d)
    hidden = shapes['embedding.weight'][1]
    px_cfg(hidden, 1 + max(int(k.split('.')[1]) for k in shapes if k.startswith('layers.')), shapes['embedding.weight'][0], classes)
    m = models.cpixelcnn()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == shapes
    assert list(m.state_dict()) == list(shapes)
    assert 'layers.1.horiz_resid.0.weight' in shapes and 'output_conv.3.weight' in shapes
    assert 'layers.0.class_cond_embedding.weight' in shapes
    assert not any('module' in k or 'codebook' in k for k in shapes)
    m.load_state_dict(gu.procedural_state_generic(shapes, seed=int(d['sd_seed'])), strict=True)


def test_exports():
    from mcgen_amd import models
    assert models.cpixelcnn and models.ConditionalGatedPixelCNN
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        import importlib
        cm = importlib.import_module('models')
        assert cm.cpixelcnn is models.cpixelcnn
        assert cm.ConditionalGatedMaskedConv2d.__name__ == 'ConditionalGatedMaskedConv2d'
        assert cm.GatedActivation.__name__ == 'GatedActivation'
    finally:
        sys.path.remove(os.path.join(ROOT, 'compat'))


def test_library_exports_cpixelcnn_kernels():
    from mcgen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.mcgen_abi_version() == 9
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = ('mcgen_cpx_gate_stats', 'mcgen_cpx_gated_fwd', 'mcgen_cpx_gated_bwd_stats', 'mcgen_cpx_gated_bwd_apply',
             'mcgen_cpx_embed_bwd', 'mcgen_cpx_gather_rows', 'mcgen_cpx_sample_row', 'mcgen_cpx_sample_col',
             'mcgen_cpx_code_embed_bwd')
    for name in names:
        assert hasattr(raw, name) and name in _lib.SYMBOLS and name in _lib.HEADER.functions, name
    # host-side argument checks, before any launch
    assert lib.mcgen_cpx_gate_stats(None, 1, 0, None) != 0
    assert b'cpx_gate_stats' in lib.mcgen_last_error()
    assert lib.mcgen_cpx_gated_fwd(None, 5, 0, None) != 0
    assert lib.mcgen_cpx_embed_bwd(None, None, None, None, 1, 32, 10, None) != 0
    assert b'cpx_embed_bwd' in lib.mcgen_last_error()
    assert lib.mcgen_cpx_gather_rows(None, None, None, 1, 1, 32, 10, None) != 0
    assert lib.mcgen_cpx_gated_bwd_stats(None, None, None, 10, None, None, None, None, None, None, None, 1, 0, 1, 1, 24, None) != 0
    assert lib.mcgen_cpx_gated_bwd_apply(None, None, None, None, 10, None, None, None, None, 1.0, None, 0, 1, 1, 16, None) != 0
    assert lib.mcgen_cpx_sample_row(None, 0, 0, None) != 0
    assert lib.mcgen_cpx_code_embed_bwd(None, 512, None, None, 64, 512, 512, 0, None) != 0      # C above 256
    assert b'cpx_code_embed_bwd' in lib.mcgen_last_error()


def test_forward_has_no_cpu_fallback(px_cfg):
    from mcgen_amd import _lib, models
    px_cfg(16, 4, 32, 10)
    m = models.cpixelcnn()
    with pytest.raises(_lib.McgenError):
        m({'img': torch.zeros(2, 8, 8, dtype=torch.long), 'label': torch.zeros(2, dtype=torch.long)})


def test_out_of_range_labels_raise(px_cfg):
    from mcgen_amd import models
    px_cfg(16, 4, 32, 10)
    m = models.cpixelcnn()
    codes = torch.zeros(1, 8, 8, dtype=torch.long)
    for bad in ([10], [-1]):
        with pytest.raises(ValueError):
            m({'img': codes, 'label': torch.tensor(bad)})
    with pytest.raises(ValueError):
        m({'img': codes, 'label': torch.tensor([1], dtype=torch.int32)})
    m.train(False)
    with pytest.raises(ValueError):
        m.sample(torch.tensor([10]))
    with pytest.raises(ValueError):
        m.sample(torch.tensor([1], dtype=torch.int32))
    m.train(True)
    with pytest.raises(ValueError):                                       # sample needs eval mode
        m.sample(torch.tensor([1]))


def test_trainer_refuses_multi_gpu(px_cfg):
    from mcgen_amd import models
    from mcgen_amd.trainer import PixelCNNTrainer
    px_cfg(16, 4, 32, 10)
    with pytest.raises(ValueError):
        PixelCNNTrainer(models.cpixelcnn(), world_size=2)


_PROBE = r'''
import json, sys
sys.path.insert(0, {compat!r})
sys.argv = ['train_pixelcnn.py'] + {args!r}
import train_pixelcnn as T
import _single
captured = {{}}
def fake_main(self):
    from utils import process_control
    process_control()
    cfg = _single.cfg
    tag = [str(cfg['init_seed']), cfg['data_name'], cfg['subset'], cfg['model_name'], cfg['control_name']]
    captured.update(tag='_'.join(x for x in tag if x), control=cfg['control'])
T.PixelCNNDriver.main = fake_main
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


def test_train_pixelcnn_cpixelcnn_tag(tmp_path):
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'cpixelcnn', '--control_name', 'None'], tmp_path)
    assert c == {'tag': '0_CIFAR10_label_cpixelcnn', 'control': {}}


def test_train_pixelcnn_keeps_mc_tags(tmp_path):
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'mcpixelcnn', '--control_name', '0.5'], tmp_path)
    assert c == {'tag': '0_CIFAR10_label_mcpixelcnn_0.5', 'control': {'controller_rate': '0.5'}}
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'mcpixelcnn'], tmp_path)
    assert c['tag'] == '0_CIFAR10_label_mcpixelcnn_0.5'
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'cvae', '--control_name', 'None'], tmp_path)
    assert c == {'error': 'Not valid model name'}
