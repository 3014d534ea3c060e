"""CGAN (models/cgan.py): module surface, parameter counts, reference checkpoints and the train_gan driver's
model-name / control handling.  CPU only."""
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
def gan_cfg():
    from mcgen_amd.config import cfg, process_control
    saved = {k: v for k, v in cfg.items()}

    def set_(data_name, g_hidden=None, d_hidden=None, classes=None):
        cfg.update(data_name=data_name, model_name='cgan', device='cpu')
        cfg.pop('classes_size', None)
        process_control()
        if classes is not None:
            cfg['classes_size'] = classes
        if g_hidden is not None:
            cfg['gan']['generator_hidden_size'], cfg['gan']['discriminator_hidden_size'] = list(g_hidden), list(d_hidden)
        return cfg
    yield set_
    cfg.clear()
    cfg.update(saved)


def _layout(d):
    """The reference's state_dict layout the fixture recorded: {key: shape}, in state_dict order."""
    out = {}
    for s in d['layout']:
        k, dims = str(s).rsplit(':', 1)
        out[k] = tuple(int(x) for x in dims.split('x')) if dims else ()
    return out


def _init_state(d):
    """The fixture's initial state: procedural weights over the recorded layout (tools/gen_golden.py)."""
    return gu.procedural_state_generic(_layout(d), seed=int(d['sd_seed']))


def _final_state(d):
    """The reference's state after training: the initial state plus the stored differences (integers stored as they are)."""
    out = {}
    for k, v in _init_state(d).items():
        if 'sd_final_int/' + k in d:
            out[k] = torch.from_numpy(np.array(d['sd_final_int/' + k]))
        else:
            out[k] = v + torch.from_numpy(d['sd_delta/' + k].astype(np.float32))
    return out


@pytest.mark.parametrize('data_name,total,g,d', [('CIFAR10', 5503236, 4408131, 1095105), ('COIL100', 8705220, None, None),
                                                 ('Omniglot', 8800258, None, None)])
def test_parameter_counts(gan_cfg, data_name, total, g, d):
    from mcgen_amd import models
    gan_cfg(data_name)
    m = models.cgan()
    assert sum(p.numel() for p in m.parameters()) == total
    if g is not None:
        assert sum(p.numel() for p in m.generator.parameters()) == g
        assert sum(p.numel() for p in m.discriminator.parameters()) == d


@pytest.mark.parametrize('fixture,data_name,classes', [('cgan_small.npz', 'CIFAR10', 10),
                                                       ('cgan_omniglot_small.npz', 'Omniglot', 1623)])
def test_state_dict_layout_and_strict_load(gan_cfg, fixture, data_name, classes):
    """The reference's state_dict layout (recorded by tools/gen_golden.py from the reference's own module tree) is exactly
    ours, key order included; a reference-layout checkpoint (after training, for cgan_small) loads with strict=True, and
    ours loads back into the same layout."""
    from mcgen_amd import models
    gan_cfg(data_name, [32] * 4, [16] * 4, classes)
    d = gu.load_npz(fixture)
    layout = _layout(d)
    m = models.cgan()
    ours = m.state_dict()
    assert list(ours) == list(layout)
    assert {k: tuple(v.shape) for k, v in ours.items()} == layout
    for k in ('discriminator.embedding.weight_orig', 'discriminator.embedding.weight_u', 'discriminator.embedding.weight_v',
              'generator.embedding.weight'):
        assert k in ours, k
    assert tuple(ours['discriminator.blocks.0.conv.0.weight_orig'].shape)[1] == (3 if data_name == 'CIFAR10' else 1) + 32
    ref = _final_state(d) if any(k.startswith('sd_delta/') for k in d) else _init_state(d)
    m.load_state_dict(ref, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, ref[k]), k
    m2 = models.cgan()
    m2.load_state_dict(m.state_dict(), strict=True)


def test_forward_has_no_cpu_fallback(gan_cfg):
    from mcgen_amd import _lib, models
    gan_cfg('CIFAR10', [32] * 4, [16] * 4, 10)
    m = models.cgan()
    with pytest.raises(_lib.McgenError):
        m.generate(torch.zeros(2, dtype=torch.long), torch.zeros(2, 128))


def test_library_exports_cgan_kernels():
    from mcgen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.mcgen_abi_version() == 9
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = ('mcgen_cgan_gen_input', 'mcgen_cgan_dis_input', 'mcgen_cgan_embed_bwd', 'mcgen_cgan_lin_dembed',
             'mcgen_cgan_dis_window_sums', 'mcgen_cgan_dis_dembed')
    for name in names:
        assert hasattr(raw, name) and name in _lib.SYMBOLS and name in _lib.HEADER.functions, name
    # host-side argument checks, before any launch
    assert lib.mcgen_cgan_gen_input(None, None, None, None, 0, 1, 128, 32, 10, 160, None) != 0
    assert b'cgan_gen_input' in lib.mcgen_last_error()
    assert lib.mcgen_cgan_embed_bwd(None, 32, None, None, 1, 32, 10, 0, None) != 0
    assert b'cgan_embed_bwd' in lib.mcgen_last_error()
    assert lib.mcgen_cgan_lin_dembed(None, None, None, 0, 1, 16, 160, 128, 24, None) != 0     # 24 does not divide 256
    assert lib.mcgen_cgan_dis_window_sums(None, None, 0, 1, 1, 1, 8, 8, None) != 0
    assert lib.mcgen_cgan_dis_dembed(None, None, None, None, None, None, None, 0, 1, 2, 8, 35, 3, 32, 1, 8, None) != 0
    assert lib.mcgen_cgan_dis_input(None, None, None, None, None, 0, 1, 1, 3, 8, 32, 10, 8, None) != 0


_PROBE = r'''
import json, sys
sys.path.insert(0, {compat!r})
sys.argv = ['train_gan.py'] + {args!r}
import train_gan as T
from config import cfg
from utils import process_control
T.parse()
process_control()
try:
    m = T.make_model()
    name = type(m).__name__
except ValueError as e:
    name = 'ValueError: ' + str(e)
print(json.dumps(dict(tag=T.model_tag(0), model=name, control=cfg['control'])))
'''


def _probe(args, tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    code = _PROBE.format(compat=os.path.join(ROOT, 'compat'), args=args)
    r = subprocess.run([sys.executable, '-c', code], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_train_gan_builds_cgan_with_empty_control(tmp_path):
    c = _probe(['--data_name', 'Omniglot', '--model_name', 'cgan', '--control_name', 'None'], tmp_path)
    assert c == {'tag': '0_Omniglot_label_cgan', 'model': 'CGAN', 'control': {}}


def test_train_gan_keeps_mcgan_tag(tmp_path):
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'mcgan', '--control_name', '0.5'], tmp_path)
    assert c == {'tag': '0_CIFAR10_label_mcgan_0.5', 'model': 'MCGAN', 'control': {'controller_rate': '0.5'}}
    c = _probe(['--data_name', 'CIFAR10'], tmp_path)                     # no --control_name: the default rate
    assert c['tag'] == '0_CIFAR10_label_mcgan_0.5' and c['model'] == 'MCGAN'


def test_train_gan_refuses_other_models(tmp_path):
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'cvae', '--control_name', 'None'], tmp_path)
    assert c['model'] == 'ValueError: Not valid model name'


def test_generate_driver_parses_none_control(tmp_path):
    code = r'''
import sys
sys.path.insert(0, {compat!r})
sys.argv = ['generate.py', '--data_name', 'Omniglot', '--model_name', 'cgan', '--control_name', 'None']
import generate as G
import _single
captured = {{}}
G.run_experiment = lambda extra: captured.update(tag=_single.cfg['model_tag'], control=_single.cfg['control'])
G.main()
print(captured['tag'], captured['control'])
'''.format(compat=os.path.join(ROOT, 'compat'))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', code], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == '0_Omniglot_label_cgan {}'


def test_eval_mode_rejects_out_of_range_labels(gan_cfg):
    """Evaluation-mode generate / discriminate check the labels on the host before any launch (ValueError), where the
    reference's F.one_hot raises."""
    from mcgen_amd import models
    gan_cfg('CIFAR10', [32] * 4, [16] * 4, 10)
    m = models.cgan()
    m.train(False)
    for bad in ([10], [-1]):
        with pytest.raises(ValueError):
            m.generate(torch.tensor(bad), torch.zeros(1, 128))
        with pytest.raises(ValueError):
            m.discriminate(torch.zeros(1, 3, 32, 32), torch.tensor(bad))
    with pytest.raises(ValueError):
        m.generate(torch.tensor([1], dtype=torch.int32), torch.zeros(1, 128))
