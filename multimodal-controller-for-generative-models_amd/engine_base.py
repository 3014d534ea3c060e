"""Host plumbing shared by the tape-and-backward engines (VAE, VQ-VAE, PixelCNN, CPixelCNN, classifier, Glow): the gradient
sink, the train / eval BatchNorm affine and the weight transposes the fused kernels take."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import ops

Tensor = torch.Tensor


def _unwrap(mod):
    """The module inside a reference `Wrapper`, or the module itself (the baselines have no wrappers)."""
    return getattr(mod, 'module', mod)


def _t1x1(w: Tensor) -> Tensor:
    """[Cout, Cin(,1,1)] -> transposed 1x1 master weight [Cin, Cout, 1, 1]."""
    return w.reshape(w.shape[0], -1).t().contiguous().reshape(-1, w.shape[0], 1, 1)


def _t3x3(w: Tensor) -> Tensor:
    """[Cout, Cin, 3, 3] -> the flipped, transposed master weight of the input-gradient convolution."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def _padv(v: Optional[Tensor], n: int) -> Optional[Tensor]:
    """A per-channel vector zero-padded to n entries (None stays None)."""
    return v if v is None or v.numel() == n else F.pad(v, (0, n - v.numel()))


class EngineBase:
    def __init__(self, model, dtype: torch.dtype = torch.float32):
        self.m = model
        self.dtype = dtype
        self._gsink = None          # id(param) -> gradient tensor while an autograd backward is collecting

    def _grad(self, p: Tensor) -> Tensor:
        """The tensor the backward accumulates p's gradient into: the autograd sink's entry, else p.grad."""
        if self._gsink is not None:
            g = self._gsink.get(id(p))
            if g is None:
                g = self._gsink[id(p)] = torch.zeros_like(p)
            return g
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        return p.grad

    def _bump(self, num_batches_tracked: Tensor) -> None:
        num_batches_tracked += 1

    def _bn(self, bn, stats: Optional[Tensor], count: int, train: bool):
        """-> (scale, shift, mean, rstd) of a BatchNorm: batch statistics (running statistics updated) in training,
        the running statistics (mean = rstd = None) in evaluation."""
        if train:
            sc, sh, mean, rstd = ops.bn_finalize(stats, count, bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                                                 bn.running_var, bn.momentum, bn.eps)
            self._bump(bn.num_batches_tracked)
            return sc, sh, mean, rstd
        sc, sh = ops.bn_eval_affine(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
        return sc, sh, None, None
