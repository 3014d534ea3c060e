"""VQ-VAE training on the HIP kernels: forward (loss, code map, reconstruction) and the hand-derived backward.
Reference chain: VQVAE.forward (vqvae.py:97-104) -> Encoder (:27-47) -> VectorQuantization.forward (modules.py:18-43)
-> Decoder (:50-75); ResBlock (vqvae.py:9-24).

The layers are MCVAE's without the MultimodalController, so the building blocks follow vae_engine.py with code=None:
* Conv2d(.., 4, 2, 1)          = strided NHWC im2col (16 taps) + the fused 1x1 convolution (bias + BN partial sums).
* ConvTranspose2d(.., 4, 2, 1) = fused 1x1 convolution producing the 16 tap planes + col2im (bias added there).
* ResBlock                     = two fused 3x3 convolutions (the second carries BN -> ReLU as its prologue)
                                 + one tail kernel  relu(BN(h2) + x).
* quantiser                    = distances from one fused 1x1 convolution over -2 E^T (bias |E|^2) in fp32, the
                                 arg-min kernel, then mcgen_vq_stats / mcgen_vq_update: the gather of q, the
                                 commitment MSE and its gradient term, and (training mode) the deterministic EMA update
                                 of the codebook buffers in place.
* loss                         = tanh + MSE in one kernel (mcgen_mse_tanh) plus vq_commit * diff.
Straight-through (quantize = input + (quantize - input).detach()): the gradient reaching the encoder's output is the
decoder input gradient plus vq_commit * 2 (f - q) / numel, which rides into the decoder's first dgrad as its `res=`.
"""
from __future__ import annotations

import torch

from . import ops
from .engine_base import _t3x3
from .ops import Seg
from .vae_engine import ConvAEEngine

Tensor = torch.Tensor


class VQVAEEngine(ConvAEEngine):
    def __init__(self, model, dtype: torch.dtype = torch.float32):
        super().__init__(model, dtype)
        if any(h % 8 for h in model.hidden_size) or model.embedding_size % 8:
            raise ValueError('Not valid hidden/embedding size: the fused path needs multiples of 8')

    @staticmethod
    def _res_parts(blk):
        """relu(BN(conv(relu(BN(conv(x))))) + x)  (vqvae.py:21-24): no controllers."""
        c = blk.conv
        return c[0], c[1], None, c[3], c[4], None

    # ---- building blocks -----------------------------------------------------------------------------------------
    def _conv3_fwd(self, conv, bn, x: Tensor, train: bool, tape, kind: str):
        """Conv3x3 (+ BN -> ReLU when `bn` is given)."""
        dt = self.dtype
        h, st = ops.conv_fused([Seg(x)], ops.prep_weight(conv.weight.detach(), dt), conv.out_channels, bias=conv.bias.detach(),
                               stats_mode=1 if (train and bn is not None) else 0)
        if bn is None:
            if tape is not None:
                tape.append(dict(kind=kind, x=x))
            return h
        n, hh, ww, _ = h.shape
        b = self._bn(bn, st, n * hh * ww, train)
        a = ops.affine_code_res(h, b[0], b[1], None, None, pre_relu=True)
        if tape is not None:
            tape.append(dict(kind=kind, x=x, h=h, bn=b))
        return a

    def _conv3_bwd(self, conv, bn, r, g: Tensor, res=None) -> Tensor:
        dt = self.dtype
        if bn is not None:
            sc, sh, mean, rstd = r['bn']
            g = ops.code_bn_bwd(g, None, r['h'], sc, mean, rstd, self._grad(bn.weight), self._grad(bn.bias), shift=sh, pre_relu=True)
        ops.wgrad(Seg(r['x']), g, conv.out_channels, conv.in_channels, self._grad(conv.weight), bias_grad=self._grad(conv.bias))
        dx, _ = ops.conv_fused([Seg(g)], ops.prep_weight(_t3x3(conv.weight.detach()), dt), conv.in_channels, res=res)
        return dx

    # ---- forward -------------------------------------------------------------------------------------------------
    def encode(self, img: Tensor, train: bool, tape):
        """-> encoder output [N, H, W, D] in the compute dtype (vqvae.py:27-47)."""
        m = self.m
        ns, nr = len(m.hidden_size), m.num_res_block
        blocks = m.encoder.blocks
        x = ops.to_nhwc(img.contiguous(), self.dtype)
        for i in range(ns):
            x = self._down_fwd(blocks[3 * i], blocks[3 * i + 1], None, x, None, train, tape)
        for r in range(nr):
            x = self._res_fwd(blocks[3 * ns + r], x, None, train, tape)
        return self._conv3_fwd(blocks[3 * ns + nr], None, x, train, tape, 'enc_out')

    def quantize(self, feat: Tensor, train: bool, want_grad: bool, want_counts: bool = False):
        """VectorQuantization.forward (modules.py:18-43) on NHWC features: -> (q [N, H, W, D] in the compute dtype,
        commitment-gradient term or None, diff device scalar, codes [N, H, W], counts or None).  Distances and the EMA
        are fp32 whatever the compute dtype; training mode updates the quantiser's buffers in place."""
        vq = self.m.quantizer
        d = self.m.embedding_size
        f32 = feat if feat.dtype == torch.float32 else feat.float()
        idx = vq._nearest(f32)
        numel = float(idx.numel() * d)
        q, g, diff, counts = ops.vq_step(f32, idx, vq.embedding, d, self.dtype, coef=self.m.vq_commit * 2.0 / numel,
                                         want_grad=want_grad, train=train, cluster_size=vq.cluster_size,
                                         embedding_mean=vq.embedding_mean, decay=vq.decay, eps=vq.eps, want_counts=want_counts)
        return q, g, diff, idx, counts

    def decode(self, q: Tensor, train: bool, tape):
        """-> pre-tanh output [N, 32, 32, pad8(C)] (vqvae.py:50-75)."""
        m = self.m
        ns, nr = len(m.hidden_size), m.num_res_block
        blocks = m.decoder.blocks
        x = self._conv3_fwd(blocks[0], blocks[1], q, train, tape, 'dec_in')
        for r in range(nr):
            x = self._res_fwd(blocks[3 + r], x, None, train, tape)
        k = 3 + nr
        for _ in range(ns - 1):
            out = self._up_fwd(blocks[k], x, tape)
            x = self._uptail_fwd(out, blocks[k + 1], None, None, train, tape)
            k += 3
        return self._up_fwd(blocks[k], x, tape)

    def forward(self, img: Tensor, train: bool, tape=None, want_grad: bool = False, want_counts: bool = False):
        """-> dict(loss, code [N, W, H], img NCHW fp32 in (-1, 1), mse, diff[, counts]) (vqvae.py:97-104)."""
        m = self.m
        feat = self.encode(img, train, tape)
        q, gq, diff, idx, counts = self.quantize(feat, train, want_grad, want_counts)
        pre = self.decode(q, train, tape)
        c = m.data_shape[0]
        numel = float(img.numel())
        target = ops.to_nhwc(img.contiguous(), torch.float32, pre.shape[-1])
        dec, sse, dpre = ops.mse_tanh(pre, target, c, 2.0 / numel, want_grad)
        mse = sse / numel
        loss = mse + m.vq_commit * diff
        if tape is not None:
            tape.append(dict(kind='loss', dpre=dpre, gq=gq))
        out = {'loss': loss, 'code': idx.transpose(1, 2), 'img': ops.to_nchw(dec, c), 'mse': mse, 'diff': diff}
        if want_counts:
            out['counts'] = counts
        return out

    # ---- backward ------------------------------------------------------------------------------------------------
    def backward(self, tape):
        m = self.m
        enc, dec = m.encoder.blocks, m.decoder.blocks
        ns, nr = len(m.hidden_size), m.num_res_block
        recs = list(tape)
        loss_rec = recs.pop()
        # decoder, last to first
        k = 3 + nr + 3 * (ns - 1)
        g = self._up_bwd(dec[k], recs.pop(), loss_rec['dpre'])
        for _ in range(ns - 1):
            k -= 3
            d_out = self._uptail_bwd(dec[k + 1], recs.pop(), g)
            g = self._up_bwd(dec[k], recs.pop(), d_out)
        for r in reversed(range(nr)):
            g = self._res_bwd(dec[3 + r], recs.pop(), g)
        # decoder input conv; the straight-through estimator adds the commitment term to its input gradient
        g = self._conv3_bwd(dec[0], dec[1], recs.pop(), g, res=loss_rec['gq'])
        # encoder
        g = self._conv3_bwd(enc[3 * ns + nr], None, recs.pop(), g)
        for r in reversed(range(nr)):
            g = self._res_bwd(enc[3 * ns + r], recs.pop(), g)
        for i in reversed(range(ns)):
            g = self._down_bwd(enc[3 * i], enc[3 * i + 1], recs.pop(), g, need_dx=(i > 0))
        assert not recs
