"""The streaming IS / FID accumulators on the device (csrc/score_ops.hip, mcgen_amd.metrics.ScoreAccumulator / GanScorer) against
their float64 restatement (tests/score_ref.py), the concatenating torch path they stand beside, and compat/train_gan.py's use of
them.

Tolerances.  Moments: exact on small integers (every partial sum is representable); on Gaussian inputs the standard bound of an
n-term float64 dot product, doubled: 2 (n + 1) u |X|^T |X| elementwise, u = 2^-53.  Covariance from raw moments: 4 n u max_j
mean(x_j^2).  Probabilities: 1e-12 relative to the sum of the absolute terms (the sums have at most 130 * 1623 terms of float64
exp / log results good to a few u each).  GanScorer against metrics.inception_score / metrics.fid on the same tensors: what
tests/test_classifier.py grants that torch path against the reference, 1e-5 absolute (IS) and 1e-3 |FID| + 1e-3."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import score_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = dict(dtype=torch.float64, device='cuda')


def _moments(parts, d, calls=1):
    """fsum, gram after `calls` passes over the row blocks `parts` (NumPy float32), from zeroed accumulators."""
    from mcgen_amd import ops
    fsum, gram = torch.zeros(d, **F64), torch.zeros(d, d, **F64)
    for _ in range(calls):
        for part in parts:
            x = torch.from_numpy(part).cuda()
            work = torch.full((ops.score_moments_work(x.shape[0], d),), float('nan'), **F64)
            ops.score_moments(x, work, fsum, gram)
    return fsum, gram


@pytest.mark.parametrize('n,d', R.MOMENT_SHAPES, ids=str)
def test_moments_exact_on_integers(n, d):
    """|x| <= 8 integers, asymmetric: a wrong fragment or accumulator layout, a missed row or column shows as an unequal integer."""
    x = R.integer_features(n, d)
    xi = torch.from_numpy(x).to(torch.int64)
    fsum, gram = _moments([x], d)
    assert torch.equal(gram.cpu(), (xi.t() @ xi).double())
    assert torch.equal(fsum.cpu(), xi.sum(0).double())
    assert torch.equal(gram, gram.t())
    fsum3, gram3 = _moments([x], d, calls=3)                                 # accumulation: three calls add three times
    assert torch.equal(gram3.cpu(), 3 * (xi.t() @ xi).double()) and torch.equal(fsum3.cpu(), 3 * xi.sum(0).double())
    assert torch.equal(gram3, gram3.t())


@pytest.mark.parametrize('n,d', R.MOMENT_SHAPES, ids=str)
def test_moments_bound_on_gaussians(n, d):
    x = R.gaussian_features(n, d)
    x64 = x.astype(np.float64)
    want, bound = x64.T @ x64, R.gram_bound(x)
    fsum, gram = _moments([x], d)
    err = np.abs(gram.cpu().numpy() - want)
    print('gram max error / bound', float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert (np.abs(fsum.cpu().numpy() - x64.sum(0)) <= 2 * (n + 1) * R.U * np.abs(x64).sum(0)).all()
    assert torch.equal(gram, gram.t())
    fsum_b, gram_b = _moments([x], d)                                         # the same call again: the same bits
    assert torch.equal(gram, gram_b) and torch.equal(fsum, fsum_b)
    _, gram3 = _moments([x], d, calls=3)
    assert torch.equal(gram3, gram3.t())
    if n > 1:                                                                # two calls on halves = one call on the whole
        fsum_h, gram_h = _moments([x[:n // 2], x[n // 2:]], d)
        assert (np.abs(gram_h.cpu().numpy() - want) <= bound).all() and torch.equal(gram_h, gram_h.t())
        assert (np.abs(fsum_h.cpu().numpy() - x64.sum(0)) <= 2 * (n + 1) * R.U * np.abs(x64).sum(0)).all()


def test_covariance_from_raw_moments():
    """Mean 10, standard deviation 0.1: the cancellation the raw-moment form costs, against float64 np.cov."""
    from mcgen_amd.metrics import ScoreAccumulator
    x = R.gaussian_features(300, 100, 10.0, 0.1)
    acc = ScoreAccumulator(2, 100, 'cuda')
    for part in (x[:130], x[130:]):
        acc.add(torch.zeros(part.shape[0], 2, device='cuda'), torch.from_numpy(part).cuda())
    n, mu, cov = acc.moments()
    want = np.cov(x.astype(np.float64), rowvar=False)
    err, bound = float(np.abs(cov.cpu().numpy() - want).max()), R.cov_bound(x)
    print('covariance from raw moments: max error', err, 'bound', bound)
    assert n == 300 and cov.dtype == torch.float64 and err <= bound
    assert float(np.abs(mu.cpu().numpy() - x.astype(np.float64).mean(0)).max()) <= 2 * (n + 1) * R.U * float(np.abs(x).mean(0).max())
    assert torch.equal(cov, cov.t())


def _probs(parts, c):
    from mcgen_amd import ops
    psum, plogp = torch.zeros(c, **F64), torch.zeros(1, **F64)
    for part in parts:
        x = torch.from_numpy(part).cuda()
        work = torch.full((ops.score_probs_work(x.shape[0], c),), float('nan'), **F64)
        ops.score_probs(x, work, psum, plogp)
    return psum, plogp


def _check_probs(x, parts):
    want_p, want_e, mass = R.probs_reference(x)
    psum, plogp = _probs(parts, x.shape[1])
    ep, ee = float(np.abs(psum.cpu().numpy() - want_p).max()), abs(float(plogp) - want_e)
    print('psum error', ep, 'of', float(want_p.max()), 'plogp error', ee, 'of', mass)
    assert (np.abs(psum.cpu().numpy() - want_p) <= 1e-12 * want_p).all()       # p >= 0: the sum of a column's absolute terms is itself
    assert ee <= 1e-12 * mass
    return psum, plogp


@pytest.mark.parametrize('n,c', R.PROB_SHAPES, ids=str)
def test_probs_against_float64(n, c):
    x = R.gaussian_logits(n, c)
    psum, plogp = _check_probs(x, [x])
    again = _probs([x], c)
    assert torch.equal(psum, again[0]) and torch.equal(plogp, again[1])      # the same bits on repetition
    if n > 1:                                                                # accumulation over two calls
        _check_probs(x, [x[:n // 3 + 1], x[n // 3 + 1:]])


def test_probs_edge_rows():
    """+-80 (the maximum must be subtracted), +-400 (p underflows to 0: 0 log 0 = 0, not NaN), a constant row."""
    x = R.edge_logits(65)
    assert (R.softmax64(x)[1] == 0).any()
    psum, plogp = _check_probs(x, [x])
    assert bool(torch.isfinite(psum).all()) and math.isfinite(float(plogp))
    _check_probs(x, [x[:2], x[2:]])


def test_probs_nan_row():
    x = R.gaussian_logits(7, 65).copy()
    x[4, 17] = float('nan')
    psum, plogp = _probs([x], 65)
    assert bool(torch.isnan(psum).all()) and math.isnan(float(plogp))


def test_wrappers_refuse_before_launch():
    from mcgen_amd import ops
    x = torch.zeros(4, 8, device='cuda')
    psum, plogp, fsum, gram = torch.zeros(8, **F64), torch.zeros(1, **F64), torch.zeros(8, **F64), torch.zeros(8, 8, **F64)
    work = torch.zeros(4096, **F64)
    cases = [
        (lambda: ops.score_probs(x.double(), work, psum, plogp), 'Not valid input'),               # wrong dtype
        (lambda: ops.score_moments(x.half(), work, fsum, gram), 'Not valid input'),
        (lambda: ops.score_probs(x.cpu(), work, psum, plogp), 'Not valid input'),                  # a CPU tensor
        (lambda: ops.score_moments(x.cpu(), work, fsum, gram), 'Not valid input'),
        (lambda: ops.score_probs(x.t(), work, psum, plogp), 'Not valid input'),                    # not contiguous
        (lambda: ops.score_probs(x, work, psum[:7], plogp), 'Not valid psum'),                     # accumulators of the wrong size
        (lambda: ops.score_probs(x, work, psum, torch.zeros(2, **F64)), 'Not valid plogp'),
        (lambda: ops.score_probs(x, work, psum.float(), plogp), 'Not valid psum'),
        (lambda: ops.score_probs(x, work, psum.cpu(), plogp), 'Not valid psum'),
        (lambda: ops.score_moments(x, work, fsum, torch.zeros(8, 7, **F64)), 'Not valid gram'),
        (lambda: ops.score_moments(x, work, torch.zeros(9, **F64), gram), 'Not valid fsum'),
        (lambda: ops.score_probs(x, work[:3], psum, plogp), 'Not valid work'),
        (lambda: ops.score_moments(x, work[:3], fsum, gram), 'Not valid work'),
        (lambda: ops.score_probs(x[:, :1].contiguous(), work, torch.zeros(1, **F64), plogp), 'Not valid input'),     # C < 2
        (lambda: ops.score_probs(x[:0], work, psum, plogp), 'Not valid input'),                    # no rows
    ]
    for call, message in cases:
        with pytest.raises(ValueError, match=message):
            call()
    torch.cuda.synchronize()
    for t in (psum, plogp, fsum, gram):                                      # nothing was launched
        assert not bool(t.any())


# ---- GanScorer --------------------------------------------------------------------------------------------------------------
def _classifier_checkpoint(path, seed=11):
    """A COIL100-configured classifier (C = 100, D = 1024) with seeded weights and non-trivial BatchNorm statistics, saved in the
    reference's checkpoint layout ({'model_dict': ...}, utils.save)."""
    from mcgen_amd import models
    from mcgen_amd.checkpoint import save
    from mcgen_amd.config import cfg, process_control
    cfg.update(data_name='COIL100', model_name='classifier', device='cuda', subset='label')
    cfg.pop('classes_size', None)
    process_control()
    torch.manual_seed(seed)
    m = models.classifier()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith('running_mean'):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith('running_var'):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
            elif k == 'classifier.weight':
                v.mul_(20.0)                                # peaked class probabilities: an InceptionScore well above 1
    os.makedirs(os.path.dirname(path), exist_ok=True)
    save({'cfg': dict(cfg), 'epoch': 2, 'model_dict': {k: v.cpu() for k, v in m.state_dict().items()}}, path)
    return path


def _images(n, seed):
    return (torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(seed)) * 2 - 1).cuda()


def test_gan_scorer_matches_the_concatenating_path(tmp_path):
    from mcgen_amd import metrics
    path = _classifier_checkpoint(str(tmp_path / 'classifier_best.pt'))
    real, generated = _images(128, 21), _images(96, 22)
    scorer = metrics.GanScorer('COIL100', real, checkpoint=path, batch_size=64)
    assert scorer.acc.classes == 100 and scorer.acc.feature_size == 1024 and scorer.real_passes == 1
    kept = scorer._real
    got = scorer.score(generated.split(40))                                  # chunks of 40, 40 and 16
    model = metrics.feature_network('COIL100', checkpoint=path, device=real.device)
    assert model is scorer.model
    want_is = metrics.inception_score(generated, 'COIL100', model=model)
    want_fid = metrics.fid(generated, 'COIL100', real=real, model=model)
    print('IS', got['InceptionScore'], want_is, 'FID', got['FID'], want_fid)
    assert set(got) == {'InceptionScore', 'FID'} and all(isinstance(v, float) for v in got.values())
    assert abs(got['InceptionScore'] - want_is) < 1e-5
    assert abs(got['FID'] - want_fid) < 1e-3 * abs(want_fid) + 1e-3
    again = scorer.score(iter(generated.split(40)))                          # a generator; the real side is not recomputed
    assert scorer.real_passes == 1 and scorer._real is kept
    assert again == got                                                      # same chunks, same order: same bits
    with torch.no_grad():                                                    # one pass gives what the two entry points give
        logits, feature = model.score_outputs({'img': generated[:40]})
        assert torch.equal(feature, model.feature({'img': generated[:40]}).float())
        assert torch.equal(logits, model({'img': generated[:40]})['label'].float())
    with pytest.raises(ValueError):
        metrics.GanScorer('CIFAR10', real)
    with pytest.raises(FileNotFoundError):
        metrics.GanScorer('COIL100', real, checkpoint=str(tmp_path / 'missing.pt'))


# ---- the driver ---------------------------------------------------------------------------------------------------------------
def _train_gan(cwd, out):
    """Two epochs on 256 seeded images read from ./data/COIL100/train.npz (the driver's own data path: with no file it says
    'synthetic stand-in' itself, and the only 'stand-in' these runs may print is the test line's)."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    rng = np.random.default_rng(31)
    os.makedirs(os.path.join(cwd, 'data', 'COIL100'))
    np.savez(os.path.join(cwd, 'data', 'COIL100', 'train.npz'), img=rng.integers(0, 256, size=(256, 32, 32, 3), dtype=np.uint8),
             label=(np.arange(256) % 100).astype(np.int64))
    return subprocess.run([sys.executable, os.path.join(ROOT, 'compat', 'train_gan.py'), '--data_name', 'COIL100', '--model_name', 'mcgan',
                           '--control_name', '0.5', '--num_epochs', '2', '--synthetic_size', '256', '--generate_per_mode', '2',
                           '--output_dir', out], cwd=cwd, env=env, capture_output=True, text=True, timeout=600)


def test_driver_scores_each_epoch_and_keeps_the_best(tmp_path):
    from mcgen_amd import checkpoint as ck
    scored, plain = tmp_path / 'scored', tmp_path / 'plain'
    scored.mkdir(), plain.mkdir()
    _classifier_checkpoint(str(scored / 'metrics_tf' / 'res' / 'classifier' / '0_COIL100_label_classifier_best.pt'))
    r = _train_gan(str(scored), str(scored / 'output'))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'stand-in' not in r.stdout and 'InceptionScore' in r.stdout and 'FID' in r.stdout
    tag = '0_COIL100_label_mcgan_0.5'
    last = ck.load(str(scored / 'output' / 'model' / f'{tag}_checkpoint.pt'))
    history = last['logger'].history
    scores, distances = history['test/InceptionScore'], history['test/FID']
    print('InceptionScore per epoch', scores, 'FID per epoch', distances)
    assert len(scores) == 2 and len(distances) == 2 and 'test/GeneratedMean' not in history
    assert all(math.isfinite(v) and 1 <= v <= 100 for v in scores) and all(math.isfinite(v) for v in distances)
    best_path = scored / 'output' / 'model' / f'{tag}_best.pt'
    assert best_path.exists()
    best = ck.load(str(best_path))
    assert best['epoch'] == (3 if scores[1] > scores[0] else 2)              # strict: a tie keeps the first epoch
    from mcgen_amd import models
    from mcgen_amd.config import cfg, process_control
    cfg.update(data_name='COIL100', model_name='mcgan', device='cuda', control={'controller_rate': '0.5'})
    cfg.pop('classes_size', None)
    process_control()
    models.mcgan().load_state_dict(best['model_dict'], strict=True)
    # without the classifier file: today's behaviour, kept
    r = _train_gan(str(plain), str(plain / 'output'))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'stand-in' in r.stdout
    assert (plain / 'output' / 'model' / f'{tag}_checkpoint.pt').exists()
    assert not (plain / 'output' / 'model' / f'{tag}_best.pt').exists()
