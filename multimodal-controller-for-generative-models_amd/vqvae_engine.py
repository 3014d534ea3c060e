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
import torch.nn.functional as F

from . import ops
from .ops import Seg, pad8

Tensor = torch.Tensor


def _t1x1(w: Tensor) -> Tensor:
    return w.reshape(w.shape[0], -1).t().contiguous().reshape(-1, w.shape[0], 1, 1)


def _t3x3(w: Tensor) -> Tensor:
    return w.flip(2, 3).transpose(0, 1).contiguous()


class VQVAEEngine:
    def __init__(self, model, dtype: torch.dtype = torch.float32):
        self.m = model
        self.dtype = dtype
        self._gsink = None
        if any(h % 8 for h in model.hidden_size) or model.embedding_size % 8:
            raise ValueError('Not valid hidden/embedding size: the fused path needs multiples of 8')

    # ---- helpers -----------------------------------------------------------------------------------------------
    def _grad(self, p: Tensor) -> Tensor:
        if self._gsink is not None:
            g = self._gsink.get(id(p))
            if g is None:
                g = self._gsink[id(p)] = torch.zeros_like(p)
            return g
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        return p.grad

    @staticmethod
    def _bn(bn, stats, count: int, train: bool):
        if train:
            sc, sh, mean, rstd = ops.bn_finalize(stats, count, bn.weight.detach(), bn.bias.detach(), bn.running_mean,
                                                 bn.running_var, bn.momentum, bn.eps)
            bn.num_batches_tracked += 1
            return sc, sh, mean, rstd
        sc, sh = ops.bn_eval_affine(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
        return sc, sh, None, None

    @staticmethod
    def _padv(v, n: int):
        return v if v is None or v.numel() == n else F.pad(v, (0, n - v.numel()))

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

    def _down_fwd(self, conv, bn, x: Tensor, train: bool, tape):
        dt = self.dtype
        cp = x.shape[-1]
        col = ops.im2col(x, 4, 4, 1, 1, stride=2)
        w = conv.weight.detach().permute(0, 2, 3, 1)                            # [co, 4, 4, ci]
        wm = F.pad(w, (0, cp - w.shape[-1])).reshape(w.shape[0], 16 * cp, 1, 1).contiguous()
        h, st = ops.conv_fused([Seg(col, ksize=1)], ops.prep_weight(wm, dt), conv.out_channels, bias=conv.bias.detach(),
                               stats_mode=1 if train else 0)
        n, ho, wo, _ = h.shape
        b = self._bn(bn, st, n * ho * wo, train)
        a = ops.affine_code_res(h, b[0], b[1], None, None, pre_relu=True)
        if tape is not None:
            tape.append(dict(kind='down', col=col, wm=wm, h=h, bn=b, cin_p=cp))
        return a

    def _down_bwd(self, conv, bn, r, g: Tensor, need_dx: bool):
        dt = self.dtype
        sc, sh, mean, rstd = r['bn']
        d_h = ops.code_bn_bwd(g, None, r['h'], sc, mean, rstd, self._grad(bn.weight), self._grad(bn.bias), shift=sh, pre_relu=True)
        co, cp = conv.out_channels, r['cin_p']
        gw = torch.empty((co, 16 * cp), dtype=torch.float32, device=g.device)
        ops.wgrad(Seg(r['col'], ksize=1), d_h, co, 16 * cp, gw, bias_grad=self._grad(conv.bias))
        self._grad(conv.weight).copy_(gw.view(co, 4, 4, cp)[..., :conv.in_channels].permute(0, 3, 1, 2))
        if not need_dx:
            return None
        wt = F.pad(_t1x1(r['wm']), (0, 0, 0, 0, 0, d_h.shape[-1] - co)).contiguous()
        dcol, _ = ops.conv_fused([Seg(d_h, ksize=1)], ops.prep_weight(wt, dt), 16 * cp)
        return ops.col2im(dcol, cp, 4, 4, 1, 1, stride=2)

    def _res_fwd(self, blk, x: Tensor, train: bool, tape):
        """relu(BN(conv(relu(BN(conv(x))))) + x)  (vqvae.py:21-24)."""
        dt = self.dtype
        conv0, bn1, conv3, bn4 = blk.conv[0], blk.conv[1], blk.conv[3], blk.conv[4]
        c = conv0.out_channels
        n, h, w, _ = x.shape
        sm = 1 if train else 0
        h1, st1 = ops.conv_fused([Seg(x)], ops.prep_weight(conv0.weight.detach(), dt), c, bias=conv0.bias.detach(), stats_mode=sm)
        b1 = self._bn(bn1, st1, n * h * w, train)
        h2, st2 = ops.conv_fused([Seg(h1, scale=b1[0], shift=b1[1], relu=True)], ops.prep_weight(conv3.weight.detach(), dt), c,
                                 bias=conv3.bias.detach(), stats_mode=sm)
        b2 = self._bn(bn4, st2, n * h * w, train)
        y = ops.affine_code_res(h2, b2[0], b2[1], None, x, post_relu=True)
        if tape is not None:
            tape.append(dict(kind='res', x=x, h1=h1, b1=b1, h2=h2, b2=b2, y=y))
        return y

    def _res_bwd(self, blk, r, g: Tensor):
        dt = self.dtype
        conv0, bn1, conv3, bn4 = blk.conv[0], blk.conv[1], blk.conv[3], blk.conv[4]
        c = conv0.out_channels
        sc2, sh2, mean2, rstd2 = r['b2']
        d_h2, g_res = ops.code_bn_bwd(g, None, r['h2'], sc2, mean2, rstd2, self._grad(bn4.weight), self._grad(bn4.bias),
                                      y_post=r['y'], want_gated=True)
        sc1, sh1, mean1, rstd1 = r['b1']
        h1, x = r['h1'], r['x']
        ops.wgrad(Seg(h1, scale=sc1, shift=sh1, relu=True), d_h2, c, c, self._grad(conv3.weight), bias_grad=self._grad(conv3.bias))
        dz1, st = ops.conv_fused([Seg(d_h2)], ops.prep_weight(_t3x3(conv3.weight.detach()), dt), c, gate_x=h1,
                                 gscale=sc1, gshift=sh1, gmean=mean1, grstd=rstd1, stats_mode=2)
        n, h, w, _ = h1.shape
        d_h1 = ops.bn_backward(st, dz1, h1, n * h * w, sc1, mean1, rstd1, self._grad(bn1.weight), self._grad(bn1.bias))
        ops.wgrad(Seg(x), d_h1, c, c, self._grad(conv0.weight), bias_grad=self._grad(conv0.bias))
        dx, _ = ops.conv_fused([Seg(d_h1)], ops.prep_weight(_t3x3(conv0.weight.detach()), dt), c, res=g_res)
        return dx

    def _up_fwd(self, convt, x: Tensor, tape):
        """ConvTranspose2d(ci, co, 4, 2, 1) -> pre-activation output [N, 2h, 2w, pad8(co)]."""
        dt = self.dtype
        co = convt.out_channels
        cop = pad8(co)
        w = convt.weight.detach().permute(2, 3, 1, 0)                           # [4, 4, co, ci]
        wm = F.pad(w, (0, 0, 0, cop - co)).reshape(16 * cop, w.shape[-1], 1, 1).contiguous()
        dcol, _ = ops.conv_fused([Seg(x, ksize=1)], ops.prep_weight(wm, dt), 16 * cop)
        out = ops.col2im(dcol, cop, 4, 4, 1, 1, stride=2, bias=convt.bias.detach())
        if tape is not None:
            tape.append(dict(kind='up', x=x, wm=wm, out=out))
        return out

    def _up_bwd(self, convt, r, d_out: Tensor, need_dx: bool = True):
        dt = self.dtype
        co, ci = convt.out_channels, convt.in_channels
        cop = d_out.shape[-1]
        ops.colsum(d_out, co, self._grad(convt.bias))
        ddcol = ops.im2col(d_out, 4, 4, 1, 1, stride=2)
        x = r['x']
        cip = x.shape[-1]
        gw = torch.empty((16 * cop, cip), dtype=torch.float32, device=d_out.device)
        ops.wgrad(Seg(x, ksize=1), ddcol, 16 * cop, cip, gw)
        self._grad(convt.weight).copy_(gw.view(4, 4, cop, cip)[:, :, :co, :ci].permute(3, 2, 0, 1))
        if not need_dx:
            return None
        dx, _ = ops.conv_fused([Seg(ddcol, ksize=1)], ops.prep_weight(_t1x1(r['wm']), dt), ci)
        return dx

    # ---- forward -------------------------------------------------------------------------------------------------
    def encode(self, img: Tensor, train: bool, tape):
        """-> encoder output [N, H, W, D] in the compute dtype (vqvae.py:27-47)."""
        m = self.m
        ns, nr = len(m.hidden_size), m.num_res_block
        blocks = m.encoder.blocks
        x = ops.to_nhwc(img.contiguous(), self.dtype)
        for i in range(ns):
            x = self._down_fwd(blocks[3 * i], blocks[3 * i + 1], x, train, tape)
        for r in range(nr):
            x = self._res_fwd(blocks[3 * ns + r], x, train, tape)
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
            x = self._res_fwd(blocks[3 + r], x, train, tape)
        k = 3 + nr
        for _ in range(ns - 1):
            out = self._up_fwd(blocks[k], x, tape)
            nb, ho, wo, cp = out.shape
            b = self._bn(blocks[k + 1], ops.channel_stats(out) if train else None, nb * ho * wo, train)
            x = ops.affine_code_res(out, self._padv(b[0], cp), self._padv(b[1], cp), None, None, pre_relu=True)
            if tape is not None:
                tape.append(dict(kind='uptail', out=out, bn=b))
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
            tail = recs.pop()
            bn = dec[k + 1]
            sc, sh, mean, rstd = tail['bn']
            cp = tail['out'].shape[-1]
            co = bn.weight.numel()
            dgam = torch.zeros(cp, dtype=torch.float32, device=g.device)
            dbet = torch.zeros(cp, dtype=torch.float32, device=g.device)
            d_out = ops.code_bn_bwd(g, None, tail['out'], self._padv(sc, cp), self._padv(mean, cp), self._padv(rstd, cp),
                                    dgam, dbet, shift=self._padv(sh, cp), pre_relu=True)
            self._grad(bn.weight).copy_(dgam[:co]); self._grad(bn.bias).copy_(dbet[:co])
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
