"""Float64 CPU references for the MCGAN kernels of csrc/small_ops.hip: spectral-norm power iteration and gradient fix,
Adam, BatchNorm statistics and backward, column sums.  Each function takes the exact values a kernel read (fp32 scalars
passed as their fp32 value, e.g. f32(0.9)) and returns float64 tensors; test_small_ops_ref_cpu.py checks them against
torch's own modules, test_mcgan_small_ops_gpu.py checks the kernels against them."""
import torch

F64 = torch.float64


def f32(x: float) -> float:
    """The fp32 value a kernel receives for the Python float x."""
    return float(torch.tensor(x, dtype=torch.float32))


def normalize(x):
    """torch.nn.functional.normalize(x, dim=0, eps=1e-12), as the kernels form it: x / max(|x|, eps)."""
    return x / max(float(x.norm()), 1e-12)


def power_v(w, u):
    """First half of a training-mode round (models/utils.py:17-21): v = normalize(W^T u); also returns W^T u."""
    vt = w.to(F64).t() @ u.to(F64)
    return normalize(vt), vt


def power_u(w, v):
    """Second half: t = W v, u = normalize(t), sigma = u . t (= |t|); returns (u, sigma, t)."""
    t = w.to(F64) @ v.to(F64)
    u = normalize(t)
    return u, float(u @ t), t


def power_round(w, u):
    """One training-mode power iteration from u -> (u', v', sigma)."""
    v, _ = power_v(w, u)
    u2, sigma, _ = power_u(w, v)
    return u2, v, sigma


def sigma_eval(w, u, v):
    """Evaluation mode: no iteration, sigma = u . (W v)."""
    return float(u.to(F64) @ (w.to(F64) @ v.to(F64)))


def grad_fix(g, w, u, v, sigma):
    """d(loss)/d(weight_orig) from d(loss)/d(W / sigma) with sigma = u^T W v and u, v held constant (torch's spectral_norm):
    (G - <G, W> / sigma * u v^T) / sigma."""
    g, w, u, v = (x.to(F64) for x in (g, w, u, v))
    d = float((g * w).sum())
    return (g - d / sigma * torch.outer(u, v)) / sigma


def adam(p, g, m, v, t, lr, b1, b2, eps, wd):
    """torch.optim.Adam's update (no amsgrad, weight decay added to the gradient) at step t -> (p', m', v')."""
    p, g, m, v = (x.to(F64) for x in (p, g, m, v))
    if wd != 0:
        g = g + wd * p
    m2 = b1 * m + (1 - b1) * g
    v2 = b2 * v + (1 - b2) * g * g
    bc1 = 1 - b1 ** t
    bc2s = (1 - b2 ** t) ** 0.5
    return p - lr / bc1 * (m2 / (v2.sqrt() / bc2s + eps)), m2, v2


def bn_stats(s1, s2, count, gamma, beta, eps):
    """Training-mode BatchNorm from a channel's sum and sum of squares -> dict of mean, biased var (clamped at 0), rstd,
    scale = gamma rstd, shift = beta - mean scale, unbiased var."""
    s1, s2, gamma, beta = (x.to(F64) for x in (s1, s2, gamma, beta))
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0.0)
    rstd = 1.0 / (var + eps).sqrt()
    scale = gamma * rstd
    unb = var * count / (count - 1) if count > 1 else var
    return {'mean': mean, 'var': var, 'rstd': rstd, 'scale': scale, 'shift': beta - mean * scale, 'unb': unb}


def bn_running(rm, rv, means, unbs, momentum):
    """Running statistics after one update per statistics group, in order (means / unbs: [groups, C])."""
    rm, rv = rm.to(F64), rv.to(F64)
    for mu, ub in zip(means, unbs):
        rm = (1 - momentum) * rm + momentum * mu.to(F64)
        rv = (1 - momentum) * rv + momentum * ub.to(F64)
    return rm, rv


def bn_eval_affine(gamma, beta, rm, rv, eps):
    """Evaluation-mode BatchNorm as an affine map -> (scale, shift)."""
    scale = gamma.to(F64) / (rv.to(F64) + eps).sqrt()
    return scale, beta.to(F64) - rm.to(F64) * scale


def bn_backward(dz, x, count, scale, mean, rstd, s1, s2, add=None):
    """dx of y = scale (x - mean) rstd + shift, channels last, from the batch sums s1 = sum dz, s2 = sum dz xhat:
    scale (dz - s1 / count - xhat s2 / count) (+ add)."""
    dz, x, scale, mean, rstd, s1, s2 = (t.to(F64) for t in (dz, x, scale, mean, rstd, s1, s2))
    xh = (x - mean) * rstd
    dx = scale * (dz - s1 / count - xh * s2 / count)
    return dx if add is None else dx + add.to(F64)


def colsum(x, c, alpha=1.0, row_perm=1):
    """alpha * sum over the leading dims of x[..., :c]; row_perm > 1 stores column j = k Cc + i at i row_perm + k."""
    s = alpha * x.to(F64).reshape(-1, x.shape[-1])[:, :c].sum(0)
    if row_perm > 1:
        s = s.view(row_perm, c // row_perm).t().reshape(-1)
    return s
