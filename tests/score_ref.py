"""Float64 NumPy restatement of the streaming IS / FID accumulators (csrc/score_ops.hip, mcgen_amd.metrics.ScoreAccumulator)
and of their finalisation, plus the seeded inputs the CPU and GPU tests share.  Nothing here imports the package."""
import functools

import numpy as np

U = 2.0 ** -53                                                      # float64 unit roundoff

MOMENT_SHAPES = [(1, 1), (3, 8), (5, 16), (4, 17), (37, 24), (67, 80), (130, 64), (300, 100), (9, 1024)]
PROB_SHAPES = [(1, 2), (3, 10), (5, 64), (7, 65), (130, 100), (33, 1623)]


def softmax64(logits):
    """Row softmax in float64 with the row maximum subtracted first."""
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def plogp_terms(p):
    """p log p elementwise with 0 log 0 = 0."""
    out = np.zeros_like(p)
    np.multiply(p, np.log(p, where=p > 0, out=np.zeros_like(p)), out=out, where=p > 0)
    return out


class RefAccumulator:
    """psum, plogp, fsum, gram and count as the kernels define them, one batch at a time."""

    def __init__(self, classes, feature_size):
        self.psum, self.plogp = np.zeros(classes), 0.0
        self.fsum, self.gram = np.zeros(feature_size), np.zeros((feature_size, feature_size))
        self.count = 0

    def add(self, logits, feature):
        p = softmax64(logits)
        x = np.asarray(feature, dtype=np.float64)
        self.psum += p.sum(axis=0)
        self.plogp += plogp_terms(p).sum()
        self.fsum += x.sum(axis=0)
        self.gram += x.T @ x
        self.count += p.shape[0]

    def inception_score(self):
        py = self.psum / self.count
        return float(np.exp(self.plogp / self.count - plogp_terms(py).sum()))

    def moments(self):
        n = self.count
        return n, self.fsum / n, (self.gram - np.outer(self.fsum, self.fsum) / n) / (n - 1)


def sqrt_psd(a):
    w, v = np.linalg.eigh((a + a.T) * 0.5)
    return (v * np.sqrt(np.clip(w, 0, None))) @ v.T


def fid_from_moments(mu1, s1, mu2, s2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), the trace through the symmetric form S1^(1/2) S2 S1^(1/2)."""
    r1 = sqrt_psd(s1)
    m = r1 @ s2 @ r1
    tr = np.sqrt(np.clip(np.linalg.eigvalsh((m + m.T) * 0.5), 0, None)).sum()
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2 * tr)


def gram_bound(x, terms=None):
    """2 (n + 1) u |X|^T |X|: the bound of an n-term float64 dot product, doubled."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    return 2 * ((x.shape[0] if terms is None else terms) + 1) * U * (a.T @ a)


def cov_bound(x):
    """4 n u max_j mean(x_j^2): what forming the covariance from raw moments costs in float64."""
    x = np.asarray(x, dtype=np.float64)
    return 4 * x.shape[0] * U * float((x * x).mean(axis=0).max())


@functools.lru_cache(maxsize=None)
def integer_features(n, d):
    """Integers in [-8, 8] as float32, no symmetry between columns: every partial sum of the moments is exact in float64."""
    return np.random.default_rng(1000 * n + d).integers(-8, 9, size=(n, d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gaussian_features(n, d, mean=0.0, std=1.0):
    return (mean + std * np.random.default_rng(7000 * n + d).standard_normal((n, d))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gaussian_logits(n, c):
    return (3.0 * np.random.default_rng(3000 * n + c).standard_normal((n, c))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def edge_logits(c=65):
    """A row of +-80 (needs the maximum subtracted), a row of +-400 (exp(-800) underflows: 0 log 0), a constant row, and two
    Gaussian rows."""
    x = gaussian_logits(5, c).copy()
    sign = np.where(np.arange(c) % 3 == 0, 1.0, -1.0).astype(np.float32)
    x[0], x[1], x[2] = 80.0 * sign, 400.0 * sign, 1.25
    return x


def probs_reference(logits):
    """(psum [C], plogp, sum |p log p|) in float64."""
    p = softmax64(logits)
    t = plogp_terms(p)
    return p.sum(axis=0), float(t.sum()), float(np.abs(t).sum())
