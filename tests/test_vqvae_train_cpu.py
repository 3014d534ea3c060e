"""CPU-side checks of the VQ-VAE training surface (no GPU): the library exports the quantiser / loss entry points, the
model's training forward has no CPU fallback, multi-GPU VQ-VAE training is refused, the driver's --control_name None
tag, and the new fixtures' step-0 records are self-consistent."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small():
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name='vqvae', device='cpu', data_shape=[3, 32, 32], compute_dtype='float32')
    cfg['vqvae'] = {'hidden_size': [16, 16], 'num_res_block': 2, 'embedding_size': 8, 'num_embedding': 64, 'vq_commit': 0.25}
    return models.vqvae()


def test_library_exports_vq_training_symbols():
    from mcgen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mcgen_vq_chunks', 'mcgen_vq_stats', 'mcgen_vq_update', 'mcgen_mse_tanh'):
        assert hasattr(raw, name) and name in _lib.SYMBOLS, name
    assert lib.mcgen_vq_chunks(8192) == 64 and lib.mcgen_vq_chunks(1000) == 8
    # host-side argument checks, before any launch
    assert lib.mcgen_vq_stats(None, None, None, None, None, None, None, None, 0.0, 0, 10, 8, 8, 64, 1, None) != 0
    assert b'vq_stats' in lib.mcgen_last_error()


def test_training_forward_has_no_cpu_fallback():
    from mcgen_amd import _lib
    m = _small()
    m.train(True)
    with pytest.raises(_lib.McgenError):
        m({'img': torch.zeros(2, 3, 32, 32)})
    with pytest.raises(NotImplementedError):                                # training-mode encode stays refused
        m.encode(torch.zeros(2, 3, 32, 32))


def test_multi_gpu_vqvae_training_is_refused():
    from mcgen_amd.trainer import VQVAETrainer
    with pytest.raises(ValueError, match='multi-GPU'):
        VQVAETrainer(_small(), world_size=2)


def test_train_vqvae_driver_refuses_other_models_and_world_size(tmp_path):
    drv = os.path.join(ROOT, 'compat', 'train_vqvae.py')
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, drv, '--model_name', 'mcvae', '--control_name', 'None'], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'Not valid model name' in r.stderr
    r = subprocess.run([sys.executable, drv, '--model_name', 'vqvae', '--control_name', 'None', '--world_size', '2'],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'world_size' in r.stderr


def test_vqvae_train_fixtures_are_consistent():
    d = gu.load_npz('vqvae_train_small.npz')
    assert abs(float(d['loss0']) - (float(d['mse0']) + 0.25 * float(d['vq0']))) < 1e-6
    assert abs(float(d['losses'][0]) - float(d['loss0'])) < 1e-12
    assert d['code0'].shape == (8, 8, 8) and len(np.unique(d['code0'])) > 32            # many codes hit
    cs = d['buf1/quantizer.cluster_size']
    counts = np.bincount(d['code0'].ravel(), minlength=64)
    assert np.allclose(cs, 0.01 * counts, rtol=1e-5, atol=1e-7)                      # decay 0.99 from zero
    f = gu.load_npz('vqvae_train_full_digest.npz')
    assert f['hist0'].sum() == 128 * 8 * 8 and f['hist0'].max() > 1000               # skewed code use under the reference init
