"""compat/create.py, compat/test_created.py and compat/transit.py as a reference user runs them, after one short epoch of
compat/train_vae.py on the synthetic on-device dataset: the created set's shape and range, the saved Davies-Bouldin index
against the float64 restatement (tests/dbi_ref.py, rtol 1e-9 as in test_dbi_gpu.py) on that very file, the transit grid, and
the refusal of a PixelCNN transit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dbi_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, 'compat')
COMMON = ['--data_name', 'CIFAR10', '--log_interval', '0.5', '--synthetic_size', '192']


def _run(args, cwd, ok=True):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, os.path.join(DRV, args[0])] + args[1:] + COMMON, cwd=cwd, env=env, capture_output=True,
                       text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


@pytest.mark.parametrize('model,control', [('cvae', 'None'), ('mcvae', '0.5')])
def test_create_score_and_transit(tmp_path, model, control):
    who = ['--model_name', model, '--control_name', control]
    tag = '_'.join(['0', 'CIFAR10', 'label', model] + ([control] if control != 'None' else []))
    _run(['train_vae.py', '--num_epochs', '1', '--batch', '64'] + who, tmp_path)
    assert (tmp_path / 'output' / 'model' / f'{tag}_best.pt').exists()
    out = _run(['create.py', '--save_npy', 'True', '--generate_per_mode', '2'] + who, tmp_path)
    assert f'Experiment: {tag}' in out and 'Not exists model tag' not in out
    created = np.load(tmp_path / 'output' / 'npy' / f'created_{tag}.npy')
    assert created.shape == (20, 3, 32, 32) and created.dtype == np.float32
    assert np.isfinite(created).all() and created.min() >= 0 and created.max() <= 255
    assert (tmp_path / 'output' / 'vis' / f'created_{tag}.npy').exists()              # the image grid (save_img)
    out = _run(['test_created.py', '--generate_per_mode', '2'] + who, tmp_path)
    saved = float(np.load(tmp_path / 'output' / 'result' / f'dbi_created_{tag}.npy', allow_pickle=True))
    want = dbi_ref.davies_bouldin(created / 255 * 2 - 1, np.tile(np.arange(10), 2))
    print(model, 'DBI', saved, want)
    assert f'Davies-Bouldin Index ({tag}): {saved}' in out
    assert abs(saved - want) <= 1e-9 * want
    _run(['transit.py', '--save_per_mode', '2'] + who, tmp_path)
    grid = np.load(tmp_path / 'output' / 'vis' / f'transited_{tag}_10.npy')
    assert grid.shape == (30, 3, 32, 32) and np.isfinite(grid).all() and np.abs(grid).max() <= 1
    # a row per alpha on one latent per mode: the column of the root (mode 0, transit.py:52) never moves, the other modes do
    assert max(np.abs(grid[10 * a] - grid[0]).max() for a in (1, 2)) < 1e-3
    assert np.abs(grid[20:] - grid[:10]).max() > 1e-3


def test_transit_refuses_pixelcnn(tmp_path):
    out = _run(['transit.py', '--model_name', 'cpixelcnn', '--control_name', 'None'], tmp_path, ok=False)
    assert 'ValueError: Not valid model name' in out
