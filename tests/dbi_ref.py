"""Float64 restatement of the Davies-Bouldin index (scikit-learn's davies_bouldin_score, which is the reference's
metrics.py:164-166 DBI), written from the definition, plus the three input cases the DBI tests, the fixture and the benchmark
check share.

    clusters     the labels present, compressed to 0 .. K-1 (an absent label id is no cluster)
    c_k          the mean of cluster k's rows
    s_k          the mean Euclidean distance of cluster k's rows to c_k
    M_kl         ||c_k - c_l||, a zero entry (the diagonal included) counting as +inf
    score        mean_k max_l (s_k + s_l) / M_kl;  0.0 when every s or every M is within 1e-8 of zero (np.allclose)
    K < 2 or K >= N: ValueError
"""
from __future__ import annotations

import numpy as np

# name -> (rows, columns, seed); the labels come from _labels below
CASES = {'uneven': (97, 48, 11), 'wide': (64, 3072, 12), 'many': (3246, 1024, 13)}


def davies_bouldin(x, label) -> float:
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    label = np.asarray(label)
    present, cluster = np.unique(label, return_inverse=True)
    k, n = len(present), len(x)
    if not 1 < k < n:
        raise ValueError('Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)' % k)
    cent = np.zeros((k, x.shape[1]))
    spread = np.zeros(k)
    for j in range(k):
        rows = x[cluster == j]
        cent[j] = rows.mean(0)
        spread[j] = np.sqrt(((rows - cent[j]) ** 2).sum(1)).mean()
    dist = np.zeros((k, k))
    for j in range(k - 1):                                       # by difference, not through the Gram matrix; M is symmetric
        diff = cent[j + 1:] - cent[j]
        dist[j, j + 1:] = dist[j + 1:, j] = np.sqrt(np.einsum('ij,ij->i', diff, diff))
    if np.allclose(spread, 0) or np.allclose(dist, 0):
        return 0.0
    dist[dist == 0] = np.inf
    return float(np.mean(np.max((spread[:, None] + spread[None, :]) / dist, axis=1)))


_REFERENCE = {}


def reference(name) -> float:
    """davies_bouldin of make_case(name), computed once per session and shared."""
    if name not in _REFERENCE:
        _REFERENCE[name] = davies_bouldin(*make_case(name))
    return _REFERENCE[name]


def _labels(name, rng):
    if name == 'uneven':           # five uneven clusters, one a singleton, with gaps in the label ids
        lab = np.repeat([0, 1, 3, 4, 7], [40, 1, 30, 20, 6])
    elif name == 'wide':           # ten clusters over the full image width
        lab = np.arange(64) % 10
    else:                          # the full Omniglot cluster count, two rows each
        lab = np.repeat(np.arange(1623), 2)
    return rng.permutation(lab).astype(np.int64)                 # rows out of label order


def make_case(name):
    """-> (x float32 [N, D], label int64 [N]): x = tanh(centre[label] + 0.5 noise), centres ~ 0.3 N(0, 1), drawn in float64
    from a fixed seed (numpy's RandomState stream is stable across versions) and rounded to float32 once."""
    n, d, seed = CASES[name]
    rng = np.random.RandomState(seed)
    label = _labels(name, rng)
    assert len(label) == n
    centre = 0.3 * rng.standard_normal((int(label.max()) + 1, d))
    x = np.tanh(centre[label] + 0.5 * rng.standard_normal((n, d)))
    return x.astype(np.float32), label
