"""Inception Score and Frechet Inception Distance from feature / probability tensors, on the device
(reference: src/metrics/metrics.py:44-161).

The reference pushes generated images through a feature network -- torchvision's pre-trained `inception_v3`
(metrics.py:64-73,116-127; weights are downloaded, which this environment cannot do) or, for COIL100 / Omniglot, the
small `models.classifier()` (metrics.py:49-62,89-113) -- then moves everything to NumPy / SciPy on the host:
`np.cov`, `scipy.linalg.sqrtm` of a 2048 x 2048 product (seconds of single-thread LAPACK per evaluation), `F.kl_div`
over the class probabilities.  This module is the part behind the network: the same statistics from tensors that stay in
HBM, in float64.  tr sqrt(S1 S2) is taken as the sum of the square roots of the eigenvalues of S1^(1/2) S2 S1^(1/2)
(symmetric positive semi-definite, so `eigh` applies) -- the quantity sqrtm's trace gives, without complex arithmetic.
"""
from __future__ import annotations

import torch


def inception_score_from_probs(pred: torch.Tensor, splits: int = 1) -> float:
    """metrics.py:75-82: pred [N, classes] softmax outputs -> mean over splits of exp(mean_n KL(p(y|x_n) || p(y)))."""
    n = pred.shape[0]
    pred = pred.to(torch.float64)
    scores = []
    for k in range(splits):
        part = pred[k * (n // splits):(k + 1) * (n // splits)]
        py = part.mean(0, keepdim=True)
        # F.kl_div(log py, part, 'batchmean') = sum part * (log part - log py) / rows, with 0 log 0 = 0
        kl = torch.where(part > 0, part * (part.clamp_min(1e-300).log() - py.log()), torch.zeros_like(part)).sum() / part.shape[0]
        scores.append(kl.exp())
    return float(torch.stack(scores).mean())


def _cov(x: torch.Tensor):
    x = x.to(torch.float64)
    mu = x.mean(0)
    xc = x - mu
    return mu, xc.t() @ xc / (x.shape[0] - 1)                      # np.cov(rowvar=False): unbiased


def _sqrt_psd(a: torch.Tensor):
    w, v = torch.linalg.eigh((a + a.t()) * 0.5)
    return (v * w.clamp_min(0).sqrt()) @ v.t()


def fid_from_features(real: torch.Tensor, generated: torch.Tensor) -> float:
    """metrics.py:139-161: |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), features [N, D] each."""
    mu1, s1 = _cov(real)
    mu2, s2 = _cov(generated)
    r1 = _sqrt_psd(s1)
    m = r1 @ s2 @ r1
    tr_covmean = torch.linalg.eigvalsh((m + m.t()) * 0.5).clamp_min(0).sqrt().sum()
    diff = mu1 - mu2
    return float(diff @ diff + torch.trace(s1) + torch.trace(s2) - 2 * tr_covmean)


# ---- the callers' entry points (metrics.py:44-81 InceptionScore, :84-161 FID) --------------------------------------
_NO_INCEPTION = ('{} on {} needs torchvision\'s pre-trained inception_v3 (metrics.py:64,116), whose weights cannot be '
                 'downloaded here; pass features to inception_score_from_probs / fid_from_features instead')


_MODEL_CACHE: dict = {}
_REAL_CACHE: dict = {}


def classifier_checkpoint_path(data_name: str, subset: str | None = 'label') -> str:
    """Where the reference keeps the feature network's weights (metrics.py:50-53,90-93):
    ./metrics_tf/res/classifier/0_<data>_<subset>_classifier_best.pt (empty tag parts dropped)."""
    tag = '_'.join(filter(None, ['0', data_name, subset, 'classifier']))
    return './metrics_tf/res/classifier/{}_best.pt'.format(tag)


def feature_network(data_name: str, checkpoint: str | None = None, device=None, subset: str | None = 'label'):
    """The feature network the reference evaluates `data_name` with: its own `models.classifier()` for COIL100 /
    Omniglot (metrics.py:49-55,89-95) on the fused convolution path, with the weights of `checkpoint` -- default: the
    reference's own location (classifier_checkpoint_path).  A missing file raises: an IS / FID from a randomly
    initialised classifier is not a metric.  Other datasets use inception_v3: ValueError.  The model is cached per
    (checkpoint file, mtime, device)."""
    if data_name not in ('COIL100', 'Omniglot'):
        raise ValueError(_NO_INCEPTION.format('IS / FID', data_name))
    import os
    from .models.classifier import classifier
    from .checkpoint import load
    path = checkpoint if checkpoint is not None else classifier_checkpoint_path(data_name, subset)
    if not os.path.exists(path):
        raise FileNotFoundError('IS / FID on {} need the trained feature classifier at {} (metrics.py:50-55; written by the '
                                "reference's train_classifier.py): refusing to score with random weights".format(data_name, path))
    key = (os.path.abspath(path), os.path.getmtime(path), str(device))
    if key not in _MODEL_CACHE:
        model = classifier()
        model.load_state_dict(load(path)['model_dict'])
        if device is not None:
            model = model.to(device)
        model.train(False)
        _MODEL_CACHE.clear()
        _MODEL_CACHE[key] = model
    return _MODEL_CACHE[key]


def inception_score(img: torch.Tensor, data_name: str, splits: int = 1, model=None, batch_size: int = 512,
                    subset: str | None = 'label') -> float:
    """metrics.py:44-81 with the class probabilities kept on the device: img [N, C, H, W] in (-1, 1)."""
    model = model if model is not None else feature_network(data_name, device=img.device, subset=subset)
    with torch.no_grad():
        pred = torch.cat([torch.softmax(model({'img': x, 'label': x.new_zeros(x.shape[0]).long()})['label'].float(), -1)
                          for x in img.split(batch_size)])
    return inception_score_from_probs(pred, splits)


def fid(img: torch.Tensor, data_name: str, real=None, model=None, batch_size: int = 512, subset: str | None = 'label') -> float:
    """metrics.py:84-161: features of the training images against those of `img` ([N, C, H, W] in (-1, 1)).  `real` is
    a tensor of images, or an iterable of collated batches {'img': ...} (the reference re-reads its train loader,
    metrics.py:88-105); its features are cached per (model, id(real))."""
    if real is None:
        raise ValueError('Not valid input: fid needs the real images (the reference re-reads its training set, metrics.py:88)')
    model = model if model is not None else feature_network(data_name, device=img.device, subset=subset)
    with torch.no_grad():
        f = lambda t: torch.cat([model.feature({'img': x}).float() for x in t.split(batch_size)])      # noqa: E731
        key = (id(model), id(real))
        if key not in _REAL_CACHE:
            if torch.is_tensor(real):
                rf = f(real)
            else:
                rf = torch.cat([model.feature({'img': b['img'].to(img.device)}).float() for b in real])
            _REAL_CACHE.clear()
            _REAL_CACHE[key] = (real, rf)           # (keeps `real` alive so the id stays unique)
        return fid_from_features(_REAL_CACHE[key][1], f(img))


# ---- streaming IS / FID: what train_gan.py:197-220 asks for after every epoch ----------------------------------------
class ScoreAccumulator:
    """The statistics behind IS and FID as float64 sums on the device that every batch adds to (csrc/score_ops.hip):
    psum [C] = column sums of softmax(logits), plogp [1] = sum p log p, fsum [D] = column sums of the features,
    gram [D, D] = their raw second moments.  Nothing is concatenated and `add` never synchronises with the host; the
    sums have a fixed order, so the same batches in the same order give the same bits."""

    def __init__(self, classes: int, feature_size: int, device):
        self.classes, self.feature_size = int(classes), int(feature_size)
        f64 = dict(dtype=torch.float64, device=device)
        self.psum, self.plogp = torch.zeros(self.classes, **f64), torch.zeros(1, **f64)
        self.fsum, self.gram = torch.zeros(self.feature_size, **f64), torch.zeros(self.feature_size, self.feature_size, **f64)
        self._work = torch.empty(0, **f64)
        self.count = 0

    def reset(self):
        for t in (self.psum, self.plogp, self.fsum, self.gram):
            t.zero_()
        self.count = 0

    def add(self, logits: torch.Tensor, feature: torch.Tensor):
        """logits [n, classes] and feature [n, feature_size] of the same n images, contiguous float32 on the device."""
        from . import ops
        if logits.dim() != 2 or feature.dim() != 2 or logits.shape[0] != feature.shape[0]:
            raise ValueError(f'Not valid input: logits {tuple(logits.shape)} and features {tuple(feature.shape)} of one batch expected')
        n = logits.shape[0]
        need = max(ops.score_probs_work(n, logits.shape[1]), ops.score_moments_work(n, feature.shape[1]))
        if self._work.numel() < need:                      # both calls are on one stream, so they can share it
            self._work = torch.empty(need, dtype=torch.float64, device=self.psum.device)
        ops.score_probs(logits, self._work, self.psum, self.plogp)
        ops.score_moments(feature, self._work, self.fsum, self.gram)
        self.count += n

    def _need(self, least: int):
        if self.count < least:
            raise ValueError(f'Not valid count: {self.count} samples accumulated, at least {least} needed')

    def inception_score_tensor(self) -> torch.Tensor:
        """exp(mean_n KL(p(y|x_n) || p(y))) = exp(plogp / N - sum_c py_c log py_c), py = psum / N: the reference's
        F.kl_div(py.log(), p, 'batchmean').exp() at splits = 1 (metrics.py:75-82 as train_gan.py calls it); float64, on the device."""
        self._need(1)
        py = self.psum / self.count
        cross = torch.where(py > 0, py * py.clamp_min(1e-300).log(), py).sum()      # (a NaN py stays a NaN)
        return (self.plogp[0] / self.count - cross).exp()

    def inception_score(self) -> float:
        return float(self.inception_score_tensor())

    def moments(self):
        """(N, mu [D], cov [D, D]) in float64 on the device; cov = (gram - fsum fsum^T / N) / (N - 1) is np.cov(rowvar=False)."""
        self._need(2)
        n = self.count
        return n, self.fsum / n, (self.gram - torch.outer(self.fsum, self.fsum) / n) / (n - 1)


def _fid_tensor(mu1, s1, mu2, s2, sqrt_s1=None) -> torch.Tensor:
    r1 = _sqrt_psd(s1) if sqrt_s1 is None else sqrt_s1
    m = r1 @ s2 @ r1
    tr_covmean = torch.linalg.eigvalsh((m + m.t()) * 0.5).clamp_min(0).sqrt().sum()
    diff = mu1 - mu2
    return diff @ diff + torch.trace(s1) + torch.trace(s2) - 2 * tr_covmean


def fid_from_moments(mu1, s1, mu2, s2, sqrt_s1=None) -> float:
    """The tail of fid_from_features from means and covariances (float64): |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2).
    `sqrt_s1` = _sqrt_psd(s1) when the caller has kept it (the real side does not change between epochs)."""
    return float(_fid_tensor(mu1, s1, mu2, s2, sqrt_s1))


class GanScorer:
    """InceptionScore and FID of a generated set as train_gan.py:197-220 computes them after every epoch, on COIL100 /
    Omniglot: the reference's small classifier (`feature_network`, which raises where it raises) run once per image for
    both metrics (`Classifier.score_outputs`), its outputs folded into a `ScoreAccumulator`.  The real set -- a tensor of
    images in (-1, 1), or an iterable of such tensors or of collated batches {'img': ...} -- goes through the same
    accumulator once, at construction; its mean, covariance and the covariance's square root are kept."""

    def __init__(self, data_name: str, real, subset: str | None = 'label', checkpoint: str | None = None, batch_size: int = 512,
                 device=None):
        if device is None:
            device = real.device if torch.is_tensor(real) else 'cuda'
        self.model = feature_network(data_name, checkpoint=checkpoint, device=device, subset=subset)
        self.batch_size = int(batch_size)
        head = self.model.classifier
        self.acc = ScoreAccumulator(head.out_features, head.in_features, device)
        self.real_passes = 0
        self._real = None
        self._real_moments(real)

    def _feed(self, chunks):
        dev = self.acc.psum.device
        with torch.no_grad():
            for chunk in ([chunks] if torch.is_tensor(chunks) else chunks):
                img = chunk['img'] if isinstance(chunk, dict) else chunk
                for x in img.to(dev).split(self.batch_size):
                    self.acc.add(*self.model.score_outputs({'img': x}))

    def _real_moments(self, real):
        self.acc.reset()
        self._feed(real)
        _, mu, cov = self.acc.moments()
        self._real = (mu, cov, _sqrt_psd(cov))
        self.real_passes += 1
        self.acc.reset()

    def score(self, chunks) -> dict:
        """chunks: an iterable of image tensors [n_i, C, H, W] in (-1, 1) (a generator is consumed as it goes: the set is
        never concatenated).  -> {'InceptionScore', 'FID'}; the one device-to-host transfer is the pair of results."""
        self.acc.reset()
        self._feed(chunks)
        _, mu2, s2 = self.acc.moments()
        mu1, s1, r1 = self._real
        both = torch.stack([self.acc.inception_score_tensor(), _fid_tensor(mu1, s1, mu2, s2, r1)])
        self.acc.reset()
        score, distance = both.tolist()
        return {'InceptionScore': score, 'FID': distance}


# ---- Davies-Bouldin index (metrics.py:164-166 DBI) -------------------------------------------------------------------
def davies_bouldin(img: torch.Tensor, label: torch.Tensor) -> float:
    """scikit-learn's davies_bouldin_score on the flattened images, computed on the device: img [N, ...] float32, label [N]
    int64, both on the GPU.  Labels are compressed to the ones present; s_k is the mean Euclidean distance of cluster k's
    rows to their mean c_k, M_kl = ||c_k - c_l|| with a zero counting as +inf, and the score is mean_k max_l (s_k + s_l) / M_kl
    -- or 0.0 when every s or every M is (allclose) zero.  Fewer than 2 clusters or as many as samples: ValueError.

    torch supplies the grouping (unique, a stable argsort, a cumulative sum); the sums run in csrc/dbi_ops.hip, in float64
    and in a fixed order, so two calls on one input return the same float.  Only that float reaches the host."""
    from . import ops
    if img.dtype != torch.float32 or not img.is_cuda:
        raise ValueError(f'Not valid input: davies_bouldin needs float32 images on the device, got {img.dtype} on {img.device}')
    if label.dtype != torch.int64 or label.dim() != 1 or label.shape[0] != img.shape[0] or label.device != img.device:
        raise ValueError('Not valid label: davies_bouldin needs one int64 label per image, on the images\' device')
    n = img.shape[0]
    x = img.reshape(n, -1).contiguous()
    present, cluster, counts = torch.unique(label, return_inverse=True, return_counts=True)
    k = present.numel()
    if not 1 < k < n:                                   # sklearn's check_number_of_labels
        raise ValueError('Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)' % k)
    cluster = cluster.contiguous()
    order = torch.argsort(cluster, stable=True)
    offset = torch.zeros(k + 1, dtype=torch.int64, device=x.device)
    offset[1:] = counts.cumsum(0)
    cent = ops.dbi_centroids(x, order, offset)
    spread = ops.dbi_spread(x, order, cluster, offset, cent)
    score, s_max, m_max = ops.dbi_score(cent, spread).tolist()
    if s_max <= 1e-8 or m_max <= 1e-8:                  # np.allclose(., 0): absolute tolerance 1e-8 on non-negative values
        return 0.0
    return score
