"""Float64 restatements of the updates of csrc/optim_ops.hip (mcgen_sgd, mcgen_rmsprop, mcgen_adamax): torch.optim's
single-tensor arithmetic with the arguments the reference passes (train_gan.py:222-236).  test_optimizers_cpu.py pins
them to torch.optim on float64 parameters; the GPU tests compare the kernels and the trainers against them.

Every function takes and returns float64 CPU tensors; state that does not exist (momentum 0) is None in and out."""
import torch

F64 = torch.float64


def _grad(p, g, wd):
    return g + wd * p if wd != 0 else g


def sgd(p, g, buf, lr, mu, wd):
    """torch.optim.SGD (no dampening, no Nesterov) -> (p', buf').  A zero buf gives torch's first step (buf = g')."""
    p, g = p.to(F64), g.to(F64)
    g = _grad(p, g, wd)
    if mu != 0:
        buf = mu * buf.to(F64) + g
        g = buf
    return p - lr * g, (buf if mu != 0 else None)


def rmsprop(p, g, sq, buf, lr, alpha, eps, mu, wd):
    """torch.optim.RMSprop (not centered) -> (p', square_avg', buf')."""
    p, g, sq = p.to(F64), g.to(F64), sq.to(F64)
    g = _grad(p, g, wd)
    sq = alpha * sq + (1 - alpha) * g * g
    q = g / (sq.sqrt() + eps)
    if mu != 0:
        buf = mu * buf.to(F64) + q
        q = buf
    return p - lr * q, sq, (buf if mu != 0 else None)


def adamax(p, g, m, u, t, lr, b1, b2, eps, wd):
    """torch.optim.Adamax at step t -> (p', exp_avg', exp_inf')."""
    p, g, m, u = (x.to(F64) for x in (p, g, m, u))
    g = _grad(p, g, wd)
    m = b1 * m + (1 - b1) * g
    u = torch.maximum(b2 * u, g.abs() + eps)
    return p - lr / (1 - b1 ** t) * (m / u), m, u
