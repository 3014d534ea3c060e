"""The device Davies-Bouldin index (mcgen_amd.metrics.davies_bouldin, csrc/dbi_ops.hip) against its float64 restatement
(tests/dbi_ref.py) on the three cases of dbi_ref.CASES: 97 x 48 in 5 uneven clusters (a singleton, gaps in the label ids),
64 x 3072 in 10 clusters (the full image width: column chunking) and 3246 x 1024 in 1623 clusters of two, shuffled (the
centroid-pair stage at its real K, rows out of label order).

Tolerance: rtol 1e-9 against float64.  The float32 inputs are read exactly and every sum is float64 over at most 3072 * N
non-negative or bounded terms, so the forward error is below n * 2^-53, about 1e-12 here; 1e-9 leaves three orders of margin
for another summation order and still catches any float32 accumulation (1e-7 at best).  The result also lies within 1e-6
relative of scikit-learn's own float32 answer (tests/golden/dbi.npz), the number a reference user would have seen."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dbi_ref
import golden_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_case(name):
    x, label = dbi_ref.make_case(name)
    return torch.from_numpy(x).cuda(), torch.from_numpy(label).cuda()


@pytest.mark.parametrize('case', list(dbi_ref.CASES))
def test_davies_bouldin_vs_float64(case):
    from mcgen_amd.metrics import davies_bouldin
    x, label = _device_case(case)
    got, want = davies_bouldin(x, label), dbi_ref.reference(case)
    seen = float(gu.load_npz('dbi.npz')[case + '/sklearn_f32'])
    print(case, got, want, abs(got - want) / want, 'scikit-learn float32', seen, abs(got - seen) / seen)
    assert isinstance(got, float)
    assert abs(got - want) <= 1e-9 * want
    assert abs(got - seen) <= 1e-6 * seen
    assert davies_bouldin(x, label) == got                                           # fixed-order sums: the identical float


def test_image_shaped_input_and_label_gaps():
    from mcgen_amd.metrics import davies_bouldin
    x, label = _device_case('uneven')
    got = davies_bouldin(x, label)
    assert davies_bouldin(x.view(97, 3, 4, 4), label) == got                         # [N, ...] is flattened
    assert davies_bouldin(x, label * 5 + 2) == got                                   # only the labels present are clusters


def test_degenerate_input_and_errors():
    from mcgen_amd.metrics import davies_bouldin
    x, label = _device_case('uneven')
    assert davies_bouldin(torch.ones_like(x), label) == 0.0
    with pytest.raises(ValueError):
        davies_bouldin(x, torch.zeros_like(label))                                   # one cluster
    with pytest.raises(ValueError):
        davies_bouldin(x, torch.arange(97).cuda())                                   # as many clusters as samples
    with pytest.raises(ValueError):
        davies_bouldin(x.double(), label)
    with pytest.raises(ValueError):
        davies_bouldin(x, label.int())
    with pytest.raises(ValueError):
        davies_bouldin(x.cpu(), label.cpu())


def test_compat_dbi_runs_on_the_device_without_scikit_learn():
    """compat.metrics.DBI on a CUDA tensor returns the device value and never imports scikit-learn (a fresh child process,
    since this one may have imported it already); a CPU tensor keeps the scikit-learn path."""
    code = '''
import sys
sys.path[:0] = [{root!r}, {tests!r}, {compat!r}]
import torch
import dbi_ref
from metrics import DBI
from mcgen_amd.metrics import davies_bouldin
x, label = dbi_ref.make_case('uneven')
x, label = torch.from_numpy(x).cuda(), torch.from_numpy(label).cuda()
got = DBI(x.view(97, 3, 4, 4), label)
assert got == davies_bouldin(x, label), got
assert not any(m == 'sklearn' or m.startswith('sklearn.') for m in sys.modules), 'scikit-learn was imported'
host = DBI(x.cpu(), label.cpu())
assert 'sklearn' in sys.modules and abs(host - got) <= 1e-6 * got, (host, got)
print('ok', got, host)
'''.format(root=ROOT, tests=os.path.join(ROOT, 'tests'), compat=os.path.join(ROOT, 'compat'))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
    assert r.returncode == 0 and 'ok' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
