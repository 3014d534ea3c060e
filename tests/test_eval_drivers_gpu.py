"""compat/test_vae.py, test_vqvae.py, test_pixelcnn.py, test_classifier.py, test_glow.py and test_generated.py as a reference
user runs them, after one short epoch of the matching train driver on the synthetic on-device dataset (200 images, batch 64: the
epoch ends in a short batch of 8, which a captured trainer runs eagerly).  Each test driver runs at --batch 80, so the last
batch has 40 rows, once with --metrics device (mcgen_amd.evaluate) and once
with --metrics host (the per-batch `Metric` loop) under the same seed: the `logger.mean['test/*']` saved to
output/result/<tag>.pt agree to 1e-5 relative (float32 torch formulas against float64 sums, test_eval_ref_cpu.py).  Every
subprocess has its own timeout and its return code is asserted before the next one starts."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, 'compat')
for p in (DRV,):
    if p not in sys.path:
        sys.path.insert(0, p)
RTOL = 1e-5

# IS and FID of a generated .npy with mcgen_amd.metrics, as compat/test_generated.py sets them up: COIL100's cfg, the classifier
# checkpoint, the 200 synthetic training images as the real set; prints one JSON line
_EXPECTED = '''
import json, sys
sys.path.insert(0, {root!r})
import numpy as np
import torch
from mcgen_amd import metrics as M
from mcgen_amd.config import cfg, process_control
from mcgen_amd.data import normalize_uint8, synthetic_uint8_dataset
cfg.update(data_name='COIL100', model_name='classifier', subset='label', device='cuda:0')
process_control()
generated = np.load({npy!r})
assert generated.shape == (200, 3, 32, 32), generated.shape
img = torch.tensor(generated / 255 * 2 - 1).cuda()
assert not torch.isnan(img).any()
model = M.feature_network('COIL100', checkpoint={ckpt!r}, device='cuda')
real, _ = synthetic_uint8_dataset(200, [3, 32, 32], 100, seed=0, device='cuda')
real = [{{'img': normalize_uint8(chunk)}} for chunk in real.split(512)]
print(json.dumps({{'is': M.inception_score(img, 'COIL100', model=model), 'fid': M.fid(img, 'COIL100', real=real, model=model)}}))
'''


def _run(args, cwd, data, ok=True, timeout=600):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    common = ['--data_name', data, '--log_interval', '0.5', '--synthetic_size', '200']
    r = subprocess.run([sys.executable, os.path.join(DRV, args[0])] + args[1:] + common, cwd=cwd, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


def _train(driver, who, cwd, data, epochs=1):
    _run([driver, '--num_epochs', str(epochs), '--batch', '64'] + who, cwd, data)


def _means(path, names):
    from utils import load
    saved = load(str(path))
    assert set(saved) == {'cfg', 'epoch', 'logger'}
    return {n: saved['logger'].mean['test/' + n] for n in names}, saved


def _device_against_host(driver, who, tag, names, cwd, data, count):
    result = cwd / 'output' / 'result' / f'{tag}.pt'
    out = _run([driver, '--batch', '80', '--metrics', 'device'] + who, cwd, data)
    assert f'Experiment: {tag}' in out and 'Not exists model tag' not in out
    device, saved = _means(result, names)
    assert saved['logger'].counter['test/' + names[0]] == count and saved['cfg']['model_tag'] == tag
    assert 'Test Epoch: {}(100%)'.format(saved['epoch']) in out
    for n in names:
        assert '{}: {:.4f}'.format(n, device[n]) in out                           # the 'test' line of Logger.write
    os.remove(result)
    _run([driver, '--batch', '80', '--metrics', 'host'] + who, cwd, data)
    host, _ = _means(result, names)
    for n in names:
        print(driver, n, 'device', device[n], 'host', host[n], abs(device[n] - host[n]) / abs(host[n]))
        assert np.isfinite(host[n]) and abs(device[n] - host[n]) <= RTOL * abs(host[n])
    return device


def _grids(cwd, tag, shape):
    for kind in ('input', 'output'):
        grid = np.load(cwd / 'output' / 'vis' / f'{kind}_{tag}.npy')
        assert grid.shape == shape and np.isfinite(grid).all(), (kind, grid.shape)


def test_test_vae(tmp_path):
    who, tag = ['--model_name', 'cvae', '--control_name', 'None'], '0_CIFAR10_label_cvae'
    _train('train_vae.py', who, tmp_path, 'CIFAR10')
    _device_against_host('test_vae.py', who, tag, ['Loss', 'BCE'], tmp_path, 'CIFAR10', 201)       # 80 + 80 + 40, then n = 1
    _grids(tmp_path, tag, (40, 3, 32, 32))


def test_test_vqvae_and_test_pixelcnn(tmp_path):
    ae, ae_tag = ['--model_name', 'vqvae', '--control_name', 'None'], '0_CIFAR10_label_vqvae'
    _train('train_vqvae.py', ae, tmp_path, 'CIFAR10')
    _device_against_host('test_vqvae.py', ae, ae_tag, ['Loss', 'MSE'], tmp_path, 'CIFAR10', 201)
    _grids(tmp_path, ae_tag, (40, 3, 32, 32))
    who, tag = ['--model_name', 'mcpixelcnn', '--control_name', '0.5'], '0_CIFAR10_label_mcpixelcnn_0.5'
    _train('train_pixelcnn.py', who, tmp_path, 'CIFAR10')
    _device_against_host('test_pixelcnn.py', who, tag, ['Loss', 'NLL'], tmp_path, 'CIFAR10', 201)
    assert not (tmp_path / 'output' / 'vis' / f'input_{tag}.npy').exists()         # test_pixelcnn.py writes no grids


def test_test_classifier(tmp_path):
    who, tag = ['--model_name', 'classifier', '--control_name', 'None'], '0_COIL100_label_classifier'
    _train('train_classifier.py', who, tmp_path, 'COIL100')
    got = _device_against_host('test_classifier.py', who, tag, ['Loss', 'Accuracy'], tmp_path, 'COIL100', 200)   # no trailing append
    assert 0.0 <= got['Accuracy'] <= 100.0


def test_test_glow(tmp_path):
    """MNIST: one input channel, the smallest Glow of the process_control table.  Eight epochs instead of one: with the
    reference's Adam 3e-4 and no warm-up the first updates throw Glow's loss from 8.28 bits/dim to 10^2 .. 10^3 (measured after
    one epoch of three steps: 183, 1029, 1167, 3567 over four runs, the reconstruction through `reverse` not finite in two of
    three), and it takes further epochs to come back (1167, 115, 26, 14, 9.5, 8.4 over six).  Evaluating the model in the
    middle of that says nothing about the drivers, so this case trains until the model is one again; everything else is as for
    the other drivers: _best.pt exists, the host value is finite, device and host agree to 1e-5, both grids are finite."""
    who, tag = ['--model_name', 'cglow', '--control_name', 'None'], '0_MNIST_label_cglow'
    _train('train_glow.py', who, tmp_path, 'MNIST', epochs=8)
    assert (tmp_path / 'output' / 'model' / f'{tag}_best.pt').exists()
    _device_against_host('test_glow.py', who, tag, ['Loss'], tmp_path, 'MNIST', 201)
    _grids(tmp_path, tag, (40, 1, 32, 32))                                         # the output is model.reverse(z) of the last batch


def test_test_generated(tmp_path):
    cls = ['--model_name', 'classifier', '--control_name', 'None']
    _train('train_classifier.py', cls, tmp_path, 'COIL100')
    os.makedirs(tmp_path / 'metrics_tf' / 'res' / 'classifier')
    shutil.copy(tmp_path / 'output' / 'model' / '0_COIL100_label_classifier_best.pt',
                tmp_path / 'metrics_tf' / 'res' / 'classifier' / '0_COIL100_label_classifier_best.pt')
    who, tag = ['--model_name', 'cvae', '--control_name', 'None'], '0_COIL100_label_cvae'
    _train('train_vae.py', who, tmp_path, 'COIL100')
    _run(['generate.py', '--save_npy', 'True', '--generate_per_mode', '2'] + who, tmp_path, 'COIL100')
    out = _run(['test_generated.py', '--generate_per_mode', '2'] + who, tmp_path, 'COIL100')
    saved = {k: float(np.load(tmp_path / 'output' / 'result' / f'{k}_generated_{tag}.npy', allow_pickle=True)) for k in ('is', 'fid')}
    assert 'Inception Score ({}): {}'.format(tag, saved['is']) in out and 'FID ({}): {}'.format(tag, saved['fid']) in out
    # the same two numbers from mcgen_amd.metrics on the same file, in a child process of its own: the feature classifier is
    # built from the process-wide cfg, which stays untouched here
    r = subprocess.run([sys.executable, '-c', _EXPECTED.format(root=ROOT, npy=str(tmp_path / 'output' / 'npy' / f'generated_{tag}.npy'),
                                                               ckpt=str(tmp_path / 'metrics_tf' / 'res' / 'classifier' /
                                                                        '0_COIL100_label_classifier_best.pt'))],
                       capture_output=True, text=True, timeout=300, cwd=tmp_path, env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    want = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ('is', 'fid'):
        print(k, saved[k], want[k], abs(saved[k] - want[k]) / abs(want[k]))
        assert np.isfinite(want[k]) and abs(saved[k] - want[k]) <= 1e-6 * abs(want[k])
    out = _run(['test_generated.py', '--generate_per_mode', '2'] + who, tmp_path, 'CIFAR10', ok=False)
    assert 'pre-trained inception_v3' in out and 'IS / FID on CIFAR10' in out
