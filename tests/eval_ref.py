"""Float64 restatement of the per-batch evaluation metrics (csrc/eval_ops.hip, mcgen_amd/evaluate.py) with torch on the CPU:
the yardstick of tests/test_eval_gpu.py.  Inputs are the float32 tensors the kernels read; everything after the read is
float64, except the (x + 1) / 2 map of BCE, which the reference does in float32 (metrics.py:24-25) and so does this.  Each log of
BCE is clamped at -100 as F.binary_cross_entropy does.  Also the input generators both test files share."""
import math

import torch

IMG_SHAPES = ([1, 1, 1, 1], [5, 3, 7, 9], [11, 3, 31, 29], [5, 3, 32, 32], [33, 1, 32, 32])
NLL_SHAPES = ((3, 37, 5, 7), (2, 512, 8, 8), (1, 2, 1, 1))
ACC_SHAPES = ((1, 10), (130, 100), (67, 1623))


def mse(out, tgt):
    d = out.double().cpu() - tgt.double().cpu()
    return float((d * d).sum() / d.numel())


def psnr(out, tgt):
    m = mse(out, tgt)
    return 20.0 * math.log10(1.0 / math.sqrt(m)) if m > 0 else float('inf')      # identical tensors: 1 / 0 = inf, as IEEE gives


def bce(out, tgt):
    o = ((out.float().cpu() + 1) / 2).double()
    t = ((tgt.float().cpu() + 1) / 2).double()
    term = -(t * torch.log(o).clamp(min=-100.0) + (1.0 - t) * torch.log(1.0 - o).clamp(min=-100.0))
    return float(term.sum() / term.numel())


def nll(logits, target):
    """F.cross_entropy(logits [N, K, ...], target [N, ...], 'mean'); a target outside [0, K) gives NaN."""
    x = logits.double().cpu().flatten(2) if logits.dim() > 2 else logits.double().cpu().unsqueeze(-1)
    t = target.cpu().reshape(x.shape[0], -1)
    if bool(((t < 0) | (t >= x.shape[1])).any()):
        return float('nan')
    m = x.max(dim=1, keepdim=True).values
    lse = torch.log(torch.exp(x - m).sum(dim=1)) + m.squeeze(1)
    return float((lse - x.gather(1, t.unsqueeze(1)).squeeze(1)).sum() / t.numel())


def accuracy(logits, label):
    """100 * hits / N: a hit is a row without NaN whose first maximum is its label; a label outside [0, C) gives NaN."""
    x, lab = logits.float().cpu(), label.cpu()
    if bool(((lab < 0) | (lab >= x.shape[1])).any()):
        return float('nan')
    hits = 0
    for row, want in zip(x.tolist(), lab.tolist()):
        if any(v != v for v in row):
            continue
        hits += row.index(max(row)) == want
    return 100.0 * hits / x.shape[0]


class Accumulator:
    """The arithmetic of DeviceEvaluator restated on the host: acc += n * v, last = v, count += n; repeat_last adds last once."""

    def __init__(self):
        self.acc, self.last, self.count = {}, {}, 0

    def update(self, values, n):
        for k, v in values.items():
            self.acc[k] = self.acc.get(k, 0.0) + n * v
            self.last[k] = v
        self.count += n

    def repeat_last(self):
        for k, v in self.last.items():
            self.acc[k] += v
        self.count += 1

    def result(self):
        return {k: a / self.count for k, a in self.acc.items()}


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def image_pair(shape, seed=0):
    """out, tgt uniform in (-1, 1); the first four elements are (o, t) = (1, 1), (-1, 1), (1, -1), (-1, -1) as far as the tensor
    reaches, so log(o) and log(1 - o) both hit the -100 clamp."""
    g = torch.Generator().manual_seed(1000 + seed)
    out = torch.rand(shape, generator=g) * 1.998 - 0.999
    tgt = torch.rand(shape, generator=g) * 1.998 - 0.999
    corners = [(1.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (-1.0, -1.0)]
    fo, ft = out.view(-1), tgt.view(-1)
    for i, (o, t) in enumerate(corners[:fo.numel()]):
        fo[i], ft[i] = o, t
    return out, tgt


def logit_map(shape, seed=0, scale=1.0):
    """logits [N, K, H, W] standard normal times `scale`, targets [N, H, W] uniform in [0, K) with 0 and K - 1 present."""
    n, k, h, w = shape
    g = torch.Generator().manual_seed(2000 + seed)
    logits = torch.randn(n, k, h, w, generator=g) * scale
    target = torch.randint(0, k, (n, h, w), generator=g)
    flat = target.view(-1)
    flat[0] = 0
    flat[-1] = k - 1 if flat.numel() > 1 else flat[-1]
    return logits, target


def class_rows(shape, seed=0):
    """logits [N, C] standard normal; about half the labels are the row's argmax, the rest are drawn at random."""
    n, c = shape
    g = torch.Generator().manual_seed(3000 + seed)
    logits = torch.randn(n, c, generator=g)
    label = torch.where(torch.rand(n, generator=g) < 0.5, logits.argmax(1), torch.randint(0, c, (n,), generator=g))
    return logits, label
