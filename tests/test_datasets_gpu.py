"""Ingested raw files on the device: a CIFAR10-format fixture (tests/datasets_fixtures.py; no Pillow involved) through
compat/data.py's fetch_dataset / make_data_loader on the GPU, and through compat/train_classifier.py end to end."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import datasets_fixtures as fx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, 'compat')


def test_loader_yields_every_ingested_image_once(tmp_path, monkeypatch):
    """One shuffled epoch at batch 128 over the 160 ingested images: a full batch and a short one, fp32 NCHW, every source
    image exactly once (matched back by label + an exact integer checksum of its bytes), every value within 1e-6 of
    (x / 255 - 0.5) / 0.5 in numpy fp32.  Both forms are two or three correctly rounded fp32 operations on magnitudes <= 1,
    so they differ by at most about 4e-7; 1e-6 is that bound with margin."""
    from mcgen_amd.config import cfg
    src = fx.cifar10(str(tmp_path / 'data' / 'CIFAR10'))
    monkeypatch.chdir(tmp_path)
    monkeypatch.syspath_prepend(COMPAT)
    import data as compat_data
    monkeypatch.setitem(cfg, 'device', 'cuda')
    monkeypatch.setitem(cfg, 'transform', None)
    monkeypatch.setitem(cfg, 'batch_size', {'train': 128, 'test': 128})
    monkeypatch.setitem(cfg, 'shuffle', {'train': True, 'test': False})
    dataset = compat_data.fetch_dataset('CIFAR10', verbose=False)
    assert (tmp_path / 'data' / 'CIFAR10' / 'train.npz').exists() and not dataset['train'].synthetic
    assert dataset['train'].img.is_cuda and dataset['train'].img.dtype == torch.uint8 and dataset['train'].classes_size == 10
    loader = compat_data.make_data_loader(dataset)['train']

    rows, labels = src['train']
    source = rows.reshape(-1, 3, 32, 32)                                           # NCHW, as the batches are
    reference = (source.astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)
    weights = np.random.default_rng(11).integers(1, 1 << 20, 3072).astype(np.int64)
    index = {(int(l), int(c)): i for i, (l, c) in enumerate(zip(labels, source.reshape(160, -1).astype(np.int64) @ weights))}
    assert len(index) == 160

    torch.manual_seed(5)
    sizes, seen, worst = [], [], 0.0
    for batch in loader:
        img, lab = batch['img'], batch['label']
        assert img.is_cuda and img.dtype == torch.float32 and tuple(img.shape[1:]) == (3, 32, 32) and lab.dtype == torch.int64
        sizes.append(img.shape[0])
        x = img.cpu().numpy()
        bytes_ = np.rint((x.astype(np.float64) + 1) * 127.5).astype(np.int64).reshape(x.shape[0], -1)
        for k, (l, c) in enumerate(zip(lab.cpu().tolist(), bytes_ @ weights)):
            i = index[(l, int(c))]
            seen.append(i)
            worst = max(worst, float(np.abs(x[k] - reference[i]).max()))
    print(f'loader vs numpy fp32 transform: max abs difference {worst:.3e}')
    assert sizes == [128, 32]
    assert sorted(seen) == list(range(160))
    assert seen != list(range(160))                                                # shuffled
    assert worst <= 1e-6


def test_train_classifier_on_ingested_raw_files(tmp_path):
    """A cwd holding only data/CIFAR10/raw: the driver ingests on first use, then trains one epoch -- one full (captured)
    batch of 128 and the short eager one of 32 -- and writes its checkpoint with a finite loss."""
    fx.cifar10(str(tmp_path / 'data' / 'CIFAR10'))
    assert os.listdir(tmp_path) == ['data'] and os.listdir(tmp_path / 'data' / 'CIFAR10') == ['raw']
    r = subprocess.run([sys.executable, os.path.join(COMPAT, 'train_classifier.py'), '--data_name', 'CIFAR10', '--model_name',
                        'classifier', '--control_name', 'None', '--num_epochs', '1'], cwd=tmp_path, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'npz (ingested from raw)' in r.stdout and 'synthetic' not in r.stdout
    assert (tmp_path / 'data' / 'CIFAR10' / 'train.npz').exists() and (tmp_path / 'data' / 'CIFAR10' / 'meta.json').exists()
    path = tmp_path / 'output' / 'model' / '0_CIFAR10_label_classifier_checkpoint.pt'
    assert path.exists()
    from mcgen_amd.checkpoint import load
    sys.path.insert(0, COMPAT)                                                     # the checkpoint pickles compat's Logger
    try:
        ckpt = load(str(path))
    finally:
        sys.path.remove(COMPAT)
    assert ckpt['epoch'] == 2 and ckpt['cfg']['classes_size'] == 10
    mean = ckpt['logger'].mean
    print('logged means:', dict(mean))
    assert math.isfinite(mean['train/Loss']) and math.isfinite(mean['test/Loss'])
    assert ckpt['logger'].counter['test/Loss'] == 160                              # both batches were seen: 128 + 32
