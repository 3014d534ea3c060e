"""The streaming IS / FID statistics on the host: the float64 restatement (tests/score_ref.py) against the reference's
formulas on the concatenated set, `metrics.fid_from_moments` against SciPy's sqrtm, the binding of csrc/score_ops.hip and the
driver's pivot rule."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_streaming_inception_score_matches_kl_div_on_the_concatenation():
    """Ragged batches (1, 37, 2, 90 rows) through the accumulator against F.kl_div(..., 'batchmean').exp() in float64 on all
    130 rows (metrics.py:75-82 at splits = 1), 1e-12 relative; and against inception_score_from_probs."""
    from mcgen_amd.metrics import inception_score_from_probs
    logits = np.concatenate([R.gaussian_logits(125, 100), R.edge_logits(100)])
    acc, at = R.RefAccumulator(100, 1), 0
    for rows in (1, 37, 2, 90):
        acc.add(logits[at:at + rows], np.zeros((rows, 1), np.float32))
        at += rows
    assert at == logits.shape[0] == acc.count
    p = torch.softmax(torch.from_numpy(logits).double(), -1)
    py = p.mean(0)
    want = float(F.kl_div(py.log().view(1, -1).expand_as(p), p, reduction='batchmean').exp())
    got = acc.inception_score()
    print('IS streaming', got, 'kl_div', want)
    assert abs(got - want) <= 1e-12 * abs(want)
    assert abs(got - inception_score_from_probs(p)) <= 1e-12 * abs(want)


@pytest.mark.parametrize('mean,std', [(0.0, 1.0), (10.0, 0.1)])
def test_covariance_from_raw_moments(mean, std):
    """cov = (gram - fsum fsum^T / N) / (N - 1) over three batches against np.cov on the whole, within 4 n u max_j mean(x_j^2)."""
    x = R.gaussian_features(300, 100, mean, std)
    acc = R.RefAccumulator(2, 100)
    for part in (x[:7], x[7:200], x[200:]):
        acc.add(np.zeros((part.shape[0], 2), np.float32), part)
    n, mu, cov = acc.moments()
    want = np.cov(x.astype(np.float64), rowvar=False)
    err = float(np.abs(cov - want).max())
    print('cov error', err, 'bound', R.cov_bound(x))
    assert n == 300 and err <= R.cov_bound(x)
    assert float(np.abs(mu - x.astype(np.float64).mean(0)).max()) <= 4 * R.U * (abs(mean) + 4 * std)


def test_fid_from_moments_matches_sqrtm():
    """Full-rank Gaussian sets (n = 300, D = 24).  FID's sensitivity to a covariance error is D |dS| / (2 sqrt(lambda_min)) with
    lambda_min about 0.5 here, so float64 rounding leaves about 1e-11; 1e-8 (tr S1 + tr S2) keeps three orders of margin."""
    from scipy import linalg
    from mcgen_amd.metrics import fid_from_moments, _sqrt_psd
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((300, 24)), 0.3 + 1.2 * rng.standard_normal((300, 24))
    mu1, s1, mu2, s2 = a.mean(0), np.cov(a, rowvar=False), b.mean(0), np.cov(b, rowvar=False)
    assert np.linalg.eigvalsh(s1).min() > 0.4 and np.linalg.eigvalsh(s2).min() > 0.4
    covmean = linalg.sqrtm(s1.dot(s2))
    want = float((mu1 - mu2).dot(mu1 - mu2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(np.real(covmean)))
    tol = 1e-8 * (np.trace(s1) + np.trace(s2))
    t = [torch.from_numpy(v) for v in (mu1, s1, mu2, s2)]
    got = fid_from_moments(*t)
    kept = fid_from_moments(*t, sqrt_s1=_sqrt_psd(t[1]))
    print('FID', got, kept, 'sqrtm', want, 'tolerance', tol)
    assert abs(got - want) <= tol and abs(kept - want) <= tol
    assert abs(R.fid_from_moments(mu1, s1, mu2, s2) - want) <= tol
    # and through raw moments: the accumulator's covariance gives the same distance
    ra, rb = R.RefAccumulator(2, 24), R.RefAccumulator(2, 24)
    ra.add(np.zeros((300, 2)), a.astype(np.float32))
    rb.add(np.zeros((300, 2)), b.astype(np.float32))
    _, m1, c1 = ra.moments()
    _, m2, c2 = rb.moments()
    a32, b32 = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    want32 = R.fid_from_moments(a32.mean(0), np.cov(a32, rowvar=False), b32.mean(0), np.cov(b32, rowvar=False))
    assert abs(R.fid_from_moments(m1, c1, m2, c2) - want32) <= tol


def test_score_symbols_are_declared_and_bound():
    from mcgen_amd import _lib
    names = ('mcgen_score_probs', 'mcgen_score_probs_work', 'mcgen_score_moments', 'mcgen_score_moments_work')
    for name in names:
        res, args = _lib.SYMBOLS[name]
        if name.endswith('_work'):
            assert res is _lib.C.c_int64 and args == [_lib.C.c_int64, _lib.C.c_int]
        else:
            assert res is _lib.C.c_int and args[-1] is _lib.C.c_void_p and args[1] is _lib.C.c_int64
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert all(hasattr(lib, name) for name in names)
        # the workspace grows with the rows up to a fixed number of slices, then stays: it bounds what a call writes
        assert lib.mcgen_score_probs_work(1, 2) == 3 and lib.mcgen_score_probs_work(10 ** 6, 100) <= 256 * 101
        assert lib.mcgen_score_moments_work(1, 1) == 1 and lib.mcgen_score_moments_work(10 ** 6, 1024) <= 128 * 1024
        assert lib.mcgen_score_probs_work(5, 1) == 0 and lib.mcgen_score_probs_work(5, 65536) == 0      # sizes the call refuses
        assert lib.mcgen_score_moments_work(0, 8) == 0
        # host-side argument checks, before any launch
        assert lib.mcgen_score_probs(None, 1, 2, None, None, None, None) != 0 and b'score_probs' in lib.mcgen_last_error()
        assert lib.mcgen_score_moments(None, 1, 2, None, None, None, None) != 0 and b'score_moments' in lib.mcgen_last_error()


def test_wrappers_refuse_host_tensors():
    from mcgen_amd import ops
    x = torch.zeros(4, 8)
    with pytest.raises(ValueError, match='Not valid input'):
        ops.score_probs(x, torch.zeros(64, dtype=torch.float64), torch.zeros(8, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match='Not valid input'):
        ops.score_moments(x, torch.zeros(64, dtype=torch.float64), torch.zeros(8, dtype=torch.float64),
                          torch.zeros(8, 8, dtype=torch.float64))


_PIVOT = r'''
import json, sys
sys.path.insert(0, {compat!r})
sys.argv = ['train_gan.py']
import train_gan as T
pivot, copied = -float('inf'), []
for value in json.loads({values!r}):
    pivot, best = T.pivot_update(pivot, value)
    copied.append(best)
print(json.dumps(dict(pivot=pivot, copied=copied)))
'''


def test_pivot_rule(tmp_path):
    """train_gan.py:29-31,119-122: the pivot starts at -inf, InceptionScore is maximised and the comparison is strict: the first
    epoch always becomes _best.pt, an equal score keeps the earlier epoch, a NaN never wins."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    values = [1.5, 1.5, 1.25, 2.0, float('nan'), 2.0, 2.5]
    code = _PIVOT.format(compat=os.path.join(ROOT, 'compat'), values=json.dumps(values))
    r = subprocess.run([sys.executable, '-c', code], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out == {'pivot': 2.5, 'copied': [True, False, False, True, False, False, True]}
