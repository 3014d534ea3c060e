"""CVAE (models/cvae.py): module surface, parameter counts, reference checkpoints, the library surface, the trainer's and
the train_vae driver's model-name / control handling.  CPU only."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def vae_cfg():
    from mcgen_amd.config import cfg
    saved = {k: v for k, v in cfg.items()}

    def set_(hidden, latent, classes, channels=3, data_name='CIFAR10'):
        cfg.update(model_name='cvae', data_name=data_name, device='cpu', classes_size=classes, data_shape=[channels, 32, 32])
        cfg['vae'] = {'hidden_size': list(hidden), 'latent_size': latent, 'num_res_block': 2, 'embedding_size': 32}
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


@pytest.mark.parametrize('data_name,classes,channels,total', [('CIFAR10', 10, 3, 7793411), ('COIL100', 100, 3, 7799171),
                                                              ('Omniglot', 1623, 1, 7892545)])
def test_parameter_counts(vae_cfg, data_name, classes, channels, total):
    from mcgen_amd import models
    vae_cfg([64, 128, 256], 128, classes, channels, data_name)
    m = models.cvae()
    assert sum(p.numel() for p in m.parameters()) == total
    assert tuple(m.encoder.embedding.weight.shape) == (32, classes) == tuple(m.decoder.embedding.weight.shape)
    assert m.encoder.blocks[0].in_channels == channels + 32 and m.decoder.linear[0].in_features == 128 + 32


@pytest.mark.parametrize('fixture,classes,channels', [('cvae_small.npz', 10, 3), ('cvae_omniglot_small.npz', 1623, 1),
                                                      ('cvae_full_digest.npz', 10, 3)])
def test_state_dict_layout_and_strict_load(vae_cfg, fixture, classes, channels):
    from mcgen_amd import models
    d = gu.load_npz(fixture)
    shapes = layout(d)
    hidden = [shapes[f'encoder.blocks.{3 * i}.weight'][0] for i in range(3)]
    vae_cfg(hidden, shapes['encoder.mu.weight'][0], classes, channels)
    m = models.cvae()
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == shapes
    assert list(m.state_dict()) == list(shapes) and len(shapes) == 106
    for k in ('encoder.embedding.weight', 'encoder.blocks.0.weight', 'decoder.linear.0.weight', 'decoder.linear.1.running_mean',
              'decoder.embedding.weight', 'encoder.blocks.9.conv.4.running_var'):
        assert k in shapes, k
    assert not any('module' in k or 'codebook' in k for k in shapes)
    m.load_state_dict(gu.procedural_state_generic(shapes, seed=int(d['sd_seed'])), strict=True)


def test_init_param_is_applied(vae_cfg):
    from mcgen_amd import models
    vae_cfg([8, 16, 32], 16, 10)
    torch.manual_seed(0)
    m = models.cvae()
    bn = m.encoder.blocks[1]
    assert float(bn.bias.detach().abs().max()) == 0.0 and 0 < float((bn.weight.detach() - 1).abs().max()) < 0.2


def test_exports():
    from mcgen_amd import models
    assert models.cvae and models.CVAE
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        import importlib
        cm = importlib.import_module('models')
        assert cm.cvae is models.cvae and cm.CVAE is models.CVAE
        assert 'cvae.py' in cm.__doc__ and '(cvae, cglow)' not in cm.__doc__
    finally:
        sys.path.remove(os.path.join(ROOT, 'compat'))


def test_library_exports_cvae_kernels():
    from mcgen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.mcgen_abi_version() == 9
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mcgen_cvae_enc_input', 'mcgen_cvae_enc_dembed', 'mcgen_cvae_latent_fwd', 'mcgen_cvae_latent_bwd'):
        assert hasattr(raw, name) and name in _lib.SYMBOLS and name in _lib.HEADER.functions, name
    # host-side argument checks, before any launch
    assert lib.mcgen_cvae_enc_input(None, None, None, None, 0, 1, 1024, 3, 32, 10, 40, None) != 0
    assert b'cvae_enc_input' in lib.mcgen_last_error()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.mcgen_cvae_enc_input(p, p, p, p, 0, 1, 1024, 3, 32, 10, 32, None) != 0          # Cp below C + E
    assert b'cvae_enc_input' in lib.mcgen_last_error()
    assert lib.mcgen_cvae_enc_input(p, p, p, p, 7, 1, 1024, 3, 32, 10, 40, None) != 0          # no such dtype
    assert b'cvae_enc_input' in lib.mcgen_last_error()
    assert lib.mcgen_cvae_enc_dembed(None, None, None, 1, 16, 64, 35, 3, 32, None) != 0
    assert b'cvae_enc_dembed' in lib.mcgen_last_error()
    assert lib.mcgen_cvae_enc_dembed(p, p, p, 1, 16, 64, 35, 3, 24, None) != 0                 # E does not divide 256
    assert lib.mcgen_cvae_enc_dembed(p, p, p, 1, 16, 64, 34, 3, 32, None) != 0                 # Cimg + E above Cin
    assert lib.mcgen_cvae_enc_dembed(p, p, p, 1, 16, 2048, 35, 3, 32, None) != 0               # beyond the LDS plan
    assert b'cvae_enc_dembed' in lib.mcgen_last_error()
    assert lib.mcgen_cvae_latent_fwd(None, 256, None, None, None, None, None, None, None, None, 0, 1, 128, 32, 10, 160, None) != 0
    assert b'cvae_latent_fwd' in lib.mcgen_last_error()
    assert lib.mcgen_cvae_latent_fwd(p, 128, None, p, p, p, p, p, p, p, 0, 1, 128, 32, 10, 160, None) != 0     # pitch below 2 L
    assert lib.mcgen_cvae_latent_fwd(p, 256, None, p, p, p, p, p, p, p, 0, 1, 128, 32, 10, 152, None) != 0     # Cp below L + E
    assert b'cvae_latent_fwd' in lib.mcgen_last_error()
    assert lib.mcgen_cvae_latent_bwd(None, 160, None, None, None, 1.0, None, None, 0, 1, 128, 32, 256, None) != 0
    assert b'cvae_latent_bwd' in lib.mcgen_last_error()
    assert lib.mcgen_cvae_latent_bwd(p, 128, p, p, p, 1.0, p, p, 0, 1, 128, 32, 256, None) != 0                # pitch below L + E
    assert lib.mcgen_cvae_latent_bwd(p, 160, p, p, p, 1.0, p, None, 0, 1, 128, 32, 256, None) != 0             # E > 0 without de
    assert b'cvae_latent_bwd' in lib.mcgen_last_error()


def test_forward_has_no_cpu_fallback(vae_cfg):
    from mcgen_amd import _lib, models
    vae_cfg([8, 16, 32], 16, 10)
    m = models.cvae()
    inp = {'img': torch.zeros(2, 3, 32, 32), 'label': torch.zeros(2, dtype=torch.long)}
    with pytest.raises(_lib.McgenError):
        m(inp)
    m.train(False)
    with pytest.raises(_lib.McgenError):
        m(inp)
    with pytest.raises(_lib.McgenError):
        m.generate(inp['label'], torch.zeros(2, 16))


def test_bad_labels_raise(vae_cfg):
    from mcgen_amd import models
    vae_cfg([8, 16, 32], 16, 10)
    m = models.cvae()
    img = torch.zeros(1, 3, 32, 32)
    for train in (True, False):
        m.train(train)
        for bad in ([10], [-1]):
            with pytest.raises(ValueError):
                m({'img': img, 'label': torch.tensor(bad)})
            with pytest.raises(ValueError):
                m.generate(torch.tensor(bad), torch.zeros(1, 16))
        with pytest.raises(ValueError):
            m({'img': img, 'label': torch.tensor([1], dtype=torch.int32)})
        with pytest.raises(ValueError):
            m({'img': img, 'label': torch.tensor([[1]])})


def test_engine_refuses_unsupported_sizes(vae_cfg):
    from mcgen_amd import models
    cfg = vae_cfg([8, 16, 32], 16, 10)
    cfg['vae']['embedding_size'] = 24
    with pytest.raises(ValueError):
        models.cvae()._engine()


def test_trainer_refuses_multi_gpu(vae_cfg):
    from mcgen_amd import models
    from mcgen_amd.trainer import VAETrainer
    vae_cfg([8, 16, 32], 16, 10)
    with pytest.raises(ValueError):
        VAETrainer(models.cvae(), world_size=2)


_PROBE = r'''
import json, sys
sys.path.insert(0, {compat!r})
sys.argv = ['train_vae.py'] + {args!r}
import train_vae as T
import _single
captured = {{}}
def fake_main(self):
    from utils import process_control
    process_control()
    cfg = _single.cfg
    tag = [str(cfg['init_seed']), cfg['data_name'], cfg['subset'], cfg['model_name'], cfg['control_name']]
    captured.update(tag='_'.join(x for x in tag if x), control=cfg['control'])
T.VAEDriver.main = fake_main
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


def test_train_vae_cvae_tag(tmp_path):
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'cvae', '--control_name', 'None'], tmp_path)
    assert c == {'tag': '0_CIFAR10_label_cvae', 'control': {}}
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'cvae', '--control_name', 'None', '--world_size', '2'], tmp_path)
    assert 'one GPU' in c['error']


def test_train_vae_keeps_mc_tags_and_refuses_other_models(tmp_path):
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'mcvae', '--control_name', '0.5'], tmp_path)
    assert c == {'tag': '0_CIFAR10_label_mcvae_0.5', 'control': {'controller_rate': '0.5'}}
    c = _probe(['--data_name', 'CIFAR10', '--model_name', 'mcvae'], tmp_path)
    assert c['tag'] == '0_CIFAR10_label_mcvae_0.5'
    for other in ('cglow', 'mcgan', 'cpixelcnn'):
        c = _probe(['--data_name', 'CIFAR10', '--model_name', other, '--control_name', 'None'], tmp_path)
        assert c == {'error': 'Not valid model name'}


def test_build_entry_is_clean_for_gfx950():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', 'import __graft_entry__ as g; g.build(); from mcgen_amd import models; print(models.cvae.__name__)'],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == 'cvae'
    assert 'cvae_ops' in open(os.path.join(ROOT, 'multimodal-controller-for-generative-models_amd', 'csrc', 'build.sh')).read()
