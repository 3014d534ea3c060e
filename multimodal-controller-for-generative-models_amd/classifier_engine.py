"""Classifier training on the HIP kernels: the training-mode forward (batch statistics) and the hand-derived backward.
Reference chain: Classifier.forward (classifier.py:45-52) -> blocks (:17-34) -> Linear (:37) -> loss (:9-11).

* stage i < 3 : Conv3x3 (fused, bias, BN partial sums, stats_mode=1) -> bn_finalize -> mcgen_affine_relu_maxpool2 with
                the batch affine sc = gamma * rstd, sh = beta - mean * sc; backward = mcgen_maxpool2_bn_bwd_{stats,apply}
                (argmax recomputed, first strict maximum, ReLU gate) -> wgrad -> dgrad (skipped for the image).
* stage 3     : Conv3x3 -> BN -> ReLU as affine_code_res(pre_relu=True); backward = code_bn_bwd(pre_relu=True).
* head        : Linear over the (c, h, w) flattening = a 1x1 convolution over the NHWC flattening with permuted columns
                (as the evaluation path); mean cross-entropy (mcgen_cross_entropy, which also writes dlogits).
                Backward: db = colsum(dlogits), dW = wgrad over N one-pixel rows (K = h * w * C), dfeat = dlogits . W as
                a 1x1 convolution over N pixels.
BatchNorm running statistics move with momentum 0.1 and the unbiased variance (bn_finalize), as in every engine here.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .engine_base import EngineBase, _t3x3
from .ops import Seg

Tensor = torch.Tensor


class ClassifierEngine(EngineBase):
    def __init__(self, model, dtype: torch.dtype = torch.float32):
        super().__init__(model, dtype)
        self.convs = [b for b in model.blocks if isinstance(b, nn.Conv2d)]
        self.bns = [b for b in model.blocks if isinstance(b, nn.BatchNorm2d)]
        if any(c.out_channels % 8 for c in self.convs):
            raise ValueError('Not valid hidden size: the fused path needs multiples of 8')

    def _head_weight(self, h: int, w: int) -> Tensor:
        """Linear weight [classes, c * h * w] -> the 1x1 weight over the NHWC flattening [classes, h * w * c, 1, 1]."""
        lin = self.m.classifier
        c = self.m.encoded_shape[0]
        return lin.weight.detach().view(lin.out_features, c, h, w).permute(0, 2, 3, 1).reshape(lin.out_features, h * w * c, 1, 1)

    # ---- forward -------------------------------------------------------------------------------------------------
    def forward(self, img: Tensor, label: Tensor, train: bool, tape=None, want_grad: bool = False):
        """-> (mean cross-entropy as a device scalar, logits [N, classes] fp32).  train: batch statistics, running
        statistics updated in place; eval: running statistics."""
        dt = self.dtype
        x = ops.to_nhwc(img.contiguous(), dt)
        last = len(self.convs) - 1
        for i, (conv, bn) in enumerate(zip(self.convs, self.bns)):
            h, st = ops.conv_fused([Seg(x)], ops.prep_weight(conv.weight.detach(), dt), conv.out_channels, bias=conv.bias.detach(),
                                   stats_mode=1 if train else 0)
            n, hh, ww, _ = h.shape
            b = self._bn(bn, st, n * hh * ww, train)
            y = ops.affine_relu_maxpool2(h, b[0], b[1]) if i < last else ops.affine_code_res(h, b[0], b[1], None, None, pre_relu=True)
            if tape is not None:
                tape.append(dict(x=x, h=h, bn=b))
            x = y
        n, hh, ww, c = x.shape
        lin = self.m.classifier
        k = hh * ww * c
        wt = self._head_weight(hh, ww).contiguous()
        feat = x.view(n, 1, 1, k)
        logits, _ = ops.conv_fused([Seg(feat, ksize=1)], ops.prep_weight(wt, dt), lin.out_features, bias=lin.bias.detach())
        rows, dl = ops.cross_entropy(logits, label, lin.out_features, want_grad)
        if tape is not None:
            tape.append(dict(feat=feat, wt=wt, dl=dl, hw=(hh, ww)))
        return rows.mean(), ops.to_nchw(logits, lin.out_features).reshape(n, lin.out_features)

    # ---- backward ------------------------------------------------------------------------------------------------
    def backward(self, tape):
        dt = self.dtype
        recs = list(tape)
        head = recs.pop()
        lin = self.m.classifier
        dl, feat, wt = head['dl'], head['feat'], head['wt']
        n, k = feat.shape[0], feat.shape[-1]
        co = lin.out_features
        hh, ww = head['hw']
        c = self.m.encoded_shape[0]
        ops.colsum(dl, co, self._grad(lin.bias))
        gw = torch.empty((co, k), dtype=torch.float32, device=dl.device)
        ops.wgrad(Seg(feat, ksize=1), dl, co, k, gw)
        self._grad(lin.weight).copy_(gw.view(co, hh, ww, c).permute(0, 3, 1, 2).reshape(co, c * hh * ww))
        # dfeat = dlogits . W: the transposed 1x1 weight, its input channels padded to dlogits' pitch
        wtt = wt.reshape(co, k).t()
        wtt = nn.functional.pad(wtt, (0, dl.shape[-1] - co)).reshape(k, dl.shape[-1], 1, 1).contiguous()
        g, _ = ops.conv_fused([Seg(dl, ksize=1)], ops.prep_weight(wtt, dt), k)
        g = g.view(n, hh, ww, c)
        last = len(self.convs) - 1
        for i in reversed(range(len(self.convs))):
            conv, bn, r = self.convs[i], self.bns[i], recs.pop()
            sc, sh, mean, rstd = r['bn']
            if i == last:
                d_h = ops.code_bn_bwd(g, None, r['h'], sc, mean, rstd, self._grad(bn.weight), self._grad(bn.bias), shift=sh,
                                      pre_relu=True)
            else:
                d_h = ops.maxpool2_bn_bwd(g, r['h'], sc, sh, mean, rstd, self._grad(bn.weight), self._grad(bn.bias))
            ops.wgrad(Seg(r['x']), d_h, conv.out_channels, conv.in_channels, self._grad(conv.weight), bias_grad=self._grad(conv.bias))
            if i > 0:
                g, _ = ops.conv_fused([Seg(d_h)], ops.prep_weight(_t3x3(conv.weight.detach()), dt), conv.in_channels)
        assert not recs
