"""CVAE on the HIP kernels: MCVAE's engine (vae_engine.py) without any MultimodalController, plus the two label embeddings
of the reference's baseline.  Reference chain: CVAE.forward (cvae.py:131-142) -> Encoder.forward (:58-67) / Decoder.forward
(:92-99) -> ResBlock.forward (:28-31), loss (:9-13).

* encoder input  = mcgen_cvae_enc_input: (img + 1) / 2 and the embedding row W_enc[:, label] broadcast over the pixels, NHWC
                   with pad8(C + E) channels in one pass; the first strided stage runs on it unchanged.
* latent         = mcgen_cvae_latent_fwd: mu, logvar, the decoder Linear's input row [z (+) W_dec[:, label]] and the KL term
                   from the mu | logvar head output; mcgen_cvae_latent_bwd packs [dmu | dlogvar] for the head's weight gradient
                   and hands out the decoder embedding's rows of the Linear's input gradient.
* encoder dE     = mcgen_cvae_enc_dembed over the window sums of the first stage's output gradient: the embedding is constant
                   over the image, so the first convolution's input gradient is never formed ("CVAE").
* dW[:, m]       = the sum of dE[n] over the samples with label m, ascending n (mcgen_cgan_embed_bwd); absent modes get 0.
The strided, residual and transposed blocks, the Linear layers and the [N, F] BatchNorm1d are VAEEngine's with code=None.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import ops
from .engine_base import _t1x1
from .ops import Seg
from .vae_engine import VAEEngine, check_train_batch

Tensor = torch.Tensor


class CVAEEngine(VAEEngine):
    def __init__(self, model, dtype: torch.dtype = torch.float32):
        super().__init__(model, dtype)
        e = model.embedding_size
        if e % 8 or 256 % e:
            raise ValueError('Not valid embedding size: the fused path needs a multiple of 8 that divides 256')
        shrink = 2 ** len(model.hidden_size)
        if model.data_shape[1] % shrink or model.data_shape[2] % shrink or model.data_shape[1] < 4 or model.data_shape[2] < 4:
            raise ValueError('Not valid data shape: every strided stage needs an even-sized input')

    @staticmethod
    def _res_parts(blk):
        """relu(BN(conv(relu(BN(conv(x))))) + x)  (cvae.py:16-31): no controllers."""
        c = blk.conv
        return c[0], c[1], None, c[3], c[4], None

    # ---- forward -------------------------------------------------------------------------------------------------
    def encode(self, img: Tensor, label: Tensor, train: bool, eps: Optional[Tensor], tape):
        """img NCHW fp32 in (-1, 1) -> (the decoder Linear's input rows [N, 1, 1, L + E], mu, logvar, kld [1])."""
        m, dt = self.m, self.dtype
        enc = m.encoder
        ns, nr = len(m.hidden_size), m.num_res_block
        x = ops.cvae_enc_input(img.contiguous(), enc.embedding.weight.detach(), label, dt)
        blocks = enc.blocks
        for i in range(ns):
            x = self._down_fwd(blocks[3 * i], blocks[3 * i + 1], None, x, None, train, tape)
        for r in range(nr):
            x = self._res_fwd(blocks[3 * ns + r], x, None, train, tape)
        n = x.shape[0]
        perm = self._flat_perm(x.device)
        flat = x.reshape(n, 1, 1, -1)
        wcat = torch.cat([enc.mu.weight.detach(), enc.logvar.weight.detach()])[:, perm].contiguous()
        bcat = torch.cat([enc.mu.bias.detach(), enc.logvar.bias.detach()])
        L = m.latent_size
        ml, _ = ops.conv_fused([Seg(flat, ksize=1)], ops.prep_weight(wcat, dt), 2 * L, bias=bcat)
        eps = eps if train else None
        mu, logvar, zrow, kld = ops.cvae_latent_fwd(ml.reshape(n, -1), eps, m.decoder.embedding.weight.detach(), label, L)
        if tape is not None:
            tape.append(dict(kind='latent', flat=flat, wcat=wcat, mu=mu, logvar=logvar, eps=eps, xshape=x.shape))
        return zrow, mu, logvar, kld

    def latent_rows(self, z: Tensor, label: Tensor) -> Tensor:
        """[N, 1, 1, L + E] in the compute dtype: a given latent z (+) W_dec[:, label] (generate, cvae.py:123-127)."""
        return ops.cgan_gen_input(z.float(), self.m.decoder.embedding.weight.detach(), label, self.dtype)

    def decode(self, zrow: Tensor, train: bool, tape):
        m, dt = self.m, self.dtype
        dec = m.decoder
        ns, nr = len(m.hidden_size), m.num_res_block
        c, h, w = dec.encoded_shape
        n = zrow.shape[0]
        perm = self._flat_perm(zrow.device)
        lin, bn1 = dec.linear[0], dec.linear[1]
        wl = lin.weight.detach()[perm].contiguous()
        a_lin, st = ops.conv_fused([Seg(zrow, ksize=1)], ops.prep_weight(wl, dt), wl.shape[0],
                                   bias=lin.bias.detach()[perm].contiguous(), stats_mode=1 if train else 0)
        # BatchNorm1d over the N samples, parameters gathered into the NHWC feature order and scattered back
        if train:
            rm, rv = bn1.running_mean[perm].contiguous(), bn1.running_var[perm].contiguous()
            sc, sh, mean, rstd = ops.bn_finalize(st, n, bn1.weight.detach()[perm].contiguous(), bn1.bias.detach()[perm].contiguous(),
                                                 rm, rv, bn1.momentum, bn1.eps)
            bn1.running_mean.index_copy_(0, perm, rm)
            bn1.running_var.index_copy_(0, perm, rv)
            bn1.num_batches_tracked += 1
        else:
            sc, sh = ops.bn_eval_affine(bn1.weight.detach()[perm].contiguous(), bn1.bias.detach()[perm].contiguous(),
                                        bn1.running_mean[perm].contiguous(), bn1.running_var[perm].contiguous(), bn1.eps)
            mean = rstd = None
        x = ops.affine_code_res(a_lin, sc, sh, None, None, pre_relu=True).reshape(n, h, w, c)
        if tape is not None:
            tape.append(dict(kind='declin', zt=zrow, wl=wl, a_lin=a_lin, bn=(sc, sh, mean, rstd)))
        blocks = dec.blocks
        for r in range(nr):
            x = self._res_fwd(blocks[r], x, None, train, tape)
        k = nr
        for _ in range(ns - 1):
            out = self._up_fwd(blocks[k], x, tape)
            x = self._uptail_fwd(out, blocks[k + 1], None, None, train, tape)
            k += 3
        return self._up_fwd(blocks[k], x, tape)                                  # logits of the final Sigmoid

    def forward(self, img: Tensor, label: Tensor, train: bool, eps: Optional[Tensor] = None, tape=None, want_grad: bool = False):
        """-> dict(loss, mu, logvar, img) with img back in (-1, 1) as NCHW fp32 (cvae.py:131-142)."""
        m = self.m
        if train:
            check_train_batch(img.shape[0])
        if train and eps is None:
            eps = torch.randn(img.shape[0], m.latent_size, device=img.device)
        zrow, mu, logvar, kld = self.encode(img, label, train, eps, tape)
        logits = self.decode(zrow, train, tape)
        numel = float(img.numel())
        c = m.data_shape[0]
        target = ops.to_nhwc(((img + 1) / 2).contiguous(), torch.float32, logits.shape[-1])
        recon, bce, dlogits = ops.bce_logits(logits, target, c, 1.0 / numel, want_grad)
        loss = (bce + kld.reshape(())) / numel
        if tape is not None:
            tape.append(dict(kind='loss', dlogits=dlogits, numel=numel))
        return {'loss': loss, 'mu': mu, 'logvar': logvar, 'img': ops.to_nchw(recon, c) * 2 - 1}

    # ---- backward ------------------------------------------------------------------------------------------------
    def backward(self, tape, label: Tensor):
        m, dt = self.m, self.dtype
        enc, dec = m.encoder, m.decoder
        ns, nr = len(m.hidden_size), m.num_res_block
        E = m.embedding_size
        recs = list(tape)
        loss_rec = recs.pop()
        numel = loss_rec['numel']
        dblocks = dec.blocks
        # decoder, last to first
        k = nr + 3 * (ns - 1)
        g = self._up_bwd(dblocks[k], recs.pop(), loss_rec['dlogits'])
        for _ in range(ns - 1):
            k -= 3
            d_out = self._uptail_bwd(dblocks[k + 1], recs.pop(), g)
            g = self._up_bwd(dblocks[k], recs.pop(), d_out)
        for r in reversed(range(nr)):
            g = self._res_bwd(dblocks[r], recs.pop(), g)
        # decoder linear: relu(BN1d(lin))  -- [N, F] tensor ops
        dl = recs.pop()
        perm = self._flat_perm(g.device)
        lin, bn1 = dec.linear[0], dec.linear[1]
        sc, sh, mean, rstd = dl['bn']
        n = g.shape[0]
        a = dl['a_lin'].reshape(n, -1).float()
        gz = g.reshape(n, -1).float() * ((a * sc + sh) > 0)
        dbeta = gz.sum(0)
        xhat = (a - mean) * rstd
        dgamma = (gz * xhat).sum(0)
        d_lin = (sc * (gz - (dbeta + xhat * dgamma) / n)).to(dt).reshape(n, 1, 1, -1).contiguous()
        self._grad(bn1.weight).index_copy_(0, perm, dgamma)
        self._grad(bn1.bias).index_copy_(0, perm, dbeta)
        F_, LE = dl['wl'].shape
        gw = torch.empty((F_, LE), dtype=torch.float32, device=g.device)
        gb = torch.empty(F_, dtype=torch.float32, device=g.device)
        ops.wgrad(Seg(dl['zt'], ksize=1), d_lin, F_, LE, gw, bias_grad=gb)
        self._grad(lin.weight).index_copy_(0, perm, gw)
        self._grad(lin.bias).index_copy_(0, perm, gb)
        dzrow, _ = ops.conv_fused([Seg(d_lin, ksize=1)], ops.prep_weight(_t1x1(dl['wl']), dt), LE)
        # latent: z = mu + eps * exp(logvar / 2), the KL term; the Linear's embedding columns are the decoder table's dE
        lat = recs.pop()
        L = m.latent_size
        dml, de = ops.cvae_latent_bwd(dzrow.reshape(n, -1), lat['mu'], lat['logvar'], lat['eps'], 1.0 / numel, E)
        ops.cgan_embed_bwd(de, label, self._grad(dec.embedding.weight))
        wcat, flat = lat['wcat'], lat['flat']
        gwc = torch.empty(wcat.shape, dtype=torch.float32, device=g.device)
        gbc = torch.empty(2 * L, dtype=torch.float32, device=g.device)
        ops.wgrad(Seg(flat, ksize=1), dml, 2 * L, wcat.shape[1], gwc, bias_grad=gbc)
        gfull = torch.empty_like(gwc)
        gfull.index_copy_(1, perm, gwc)
        self._grad(enc.mu.weight).copy_(gfull[:L]); self._grad(enc.logvar.weight).copy_(gfull[L:])
        self._grad(enc.mu.bias).copy_(gbc[:L]); self._grad(enc.logvar.bias).copy_(gbc[L:])
        wt = F.pad(_t1x1(wcat), (0, 0, 0, 0, 0, dml.shape[-1] - 2 * L)).contiguous()
        g, _ = ops.conv_fused([Seg(dml, ksize=1)], ops.prep_weight(wt, dt), wcat.shape[1])
        g = g.reshape(lat['xshape'])
        # encoder
        eblocks = enc.blocks
        for r in reversed(range(nr)):
            g = self._res_bwd(eblocks[3 * ns + r], recs.pop(), g)
        for i in reversed(range(1, ns)):
            g = self._down_bwd(eblocks[3 * i], eblocks[3 * i + 1], recs.pop(), g, need_dx=True)
        # first stage: its weight gradient, and the encoder table's dE from its output gradient alone
        conv0 = eblocks[0]
        _, d_h = self._down_bwd(conv0, eblocks[1], recs.pop(), g, need_dx=False, want_dh=True)
        de = ops.cvae_enc_dembed(d_h, conv0.weight.detach(), m.data_shape[0], E)
        ops.cgan_embed_bwd(de, label, self._grad(enc.embedding.weight))
        assert not recs
