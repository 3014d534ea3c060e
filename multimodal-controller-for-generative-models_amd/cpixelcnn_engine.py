"""ConditionalGatedPixelCNN on the HIP kernels: PixelCNNEngine's convolution chain with every MultimodalController code
absent and the per-label embedding row of each layer added to both gate inputs.
Reference chain: ConditionalGatedPixelCNN.forward (cpixelcnn.py:86-98) -> ConditionalGatedMaskedConv2d.forward (:46-62) ->
GatedActivation.forward (:14-18).

Per layer (C = hidden, e_n = class_cond_embedding.weight[label_n], 2C channels):
  h_vert, s = vert_stack(x_v), vert_to_horiz(h_vert) + horiz_stack(x_h)      the MCPixelCNN launches, no epilogue statistics
  BatchNorm statistics of h_vert[:, :C] + e[:C] and s[:, :C] + e[:C]       one launch for both gates (mcgen_cpx_gate_stats)
  out_v, out_h = gate(h_vert + e), gate(s + e)                             one launch; the row is added in the kernel, so
                                                                           h_vert stays unbiased for vert_to_horiz
  x_h'  = BN(conv1x1(out_h)) (+ x_h)
Head: conv1x1 -> BN -> ReLU folded into the prologue of the final conv1x1.
Backward: the gate backward also leaves the per-image channel sums of its input gradient; the embedding gradient is their
per-label sum (mcgen_cpx_embed_bwd), so it needs no extra pass over the activations.  The code embedding's gradient is a
fixed-order per-code sum (mcgen_cpx_code_embed_bwd): no reduction of the step uses float atomics, so graph replays repeat
the eager step bit for bit.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import ops
from .ops import Seg
from .pixelcnn_engine import PixelCNNEngine, _t1x1

Tensor = torch.Tensor


class CPixelCNNEngine(PixelCNNEngine):

    # ---- forward ------------------------------------------------------------------------------------------------
    def _layer_forward(self, L, x_v: Tensor, x_h: Tensor, label: Tensor, train: bool, tape, I, li):
        dt = self.dtype
        n, h, w, c = x_v.shape
        count = n * h * w
        if L.mask_type == 'A':
            L.make_causal()                                   # zeroes the parameters in place, as the reference does
        k2 = L.kernel // 2
        if L.kernel == 3:
            wv = wh = None
            in_v, in_h = Seg(x_v), Seg(x_h)
            img_v, img_h = I[(li, 'v')], I[(li, 'h')]
        else:
            wv, wh = self._stack_weights(L)
            in_v = Seg(ops.im2col(x_v, k2 + 1, L.kernel, k2, k2), ksize=1)
            in_h = Seg(ops.im2col(x_h, 1, k2 + 1, 0, k2), ksize=1)
            img_v, img_h = ops.prep_weight(wv, dt), ops.prep_weight(wh, dt)
        h_vert, _ = ops.conv_fused([in_v], img_v, 2 * c, bias=L.vert_stack.bias.detach())
        wimg = I.get((li, 'v2h+h'))
        if wimg is None:
            wimg = torch.cat([I[(li, 'v2h')], img_h])
        s, _ = ops.conv_fused([Seg(h_vert, ksize=1), in_h], wimg, 2 * c,
                              bias=L.vert_to_horiz.bias.detach(), bias2=L.horiz_stack.bias.detach())
        emb = L.class_cond_embedding.weight.detach()
        bv, bh = L.gate_v.bn, L.gate_h.bn
        if train:
            # the statistics of the BIASED inputs (the conv epilogue's would be those of h_vert / s): one launch for both gates
            st_v, st_s = ops.cpx_gate_stats([(h_vert, emb, label), (s, emb, label)])
            bn_v, bn_h = ops.bn_finalize_batch([
                (st_v, count, bv.weight.detach(), bv.bias.detach(), bv.running_mean, bv.running_var, bv.momentum, bv.eps),
                (st_s, count, bh.weight.detach(), bh.bias.detach(), bh.running_mean, bh.running_var, bh.momentum, bh.eps)])
            self._nbt += [bv.num_batches_tracked, bh.num_batches_tracked]
        else:
            bn_v = self._bn(bv, None, count, False)
            bn_h = self._bn(bh, None, count, False)
        out_v, out_h = ops.cpx_gated_fwd([(h_vert, emb, label, bn_v[0], bn_v[1]), (s, emb, label, bn_h[0], bn_h[1])])
        conv_r, bn_rm = L.horiz_resid[0], L.horiz_resid[1]
        r, st_r = ops.conv_fused([Seg(out_h, ksize=1)], I[(li, 'r')], c, bias=conv_r.bias.detach(), stats_mode=1 if train else 0)
        bn_r = self._bn(bn_rm, st_r, count, train)
        x_h_new = ops.affine_code_res(r, bn_r[0], bn_r[1], None, x_h if L.residual else None)
        if tape is not None:
            tape.append(dict(in_v=in_v, in_h=in_h, h_vert=h_vert, s=s, out_h=out_h, r=r, bn_v=bn_v, bn_h=bn_h, bn_r=bn_r,
                             wv=wv, wh=wh))
        return out_v, x_h_new

    def forward(self, codes: Tensor, label: Tensor, train: bool, tape=None, want_grad: bool = False):
        """-> (loss, logits NHWC, dlogits or None).  `codes` int64 [N, H, W], `label` int64 [N] inside [0, num_mode)."""
        m, dt = self.m, self.dtype
        n, h, w = codes.shape
        x = F.embedding(codes, m.embedding.weight.detach()).to(dt).contiguous()           # [N, H, W, C] is already NHWC
        x_v = x_h = x
        layers = [] if tape is not None else None
        self._nbt = []
        I = self._images(False)
        for li, L in enumerate(m.layers):
            x_v, x_h = self._layer_forward(L, x_v, x_h, label, train, layers, I, li)
        oc = m.output_conv
        conv0, bn0, conv3 = oc[0], oc[1], oc[3]
        h0, st0 = ops.conv_fused([Seg(x_h, ksize=1)], I[('head', 0)], conv0.out_channels,
                                 bias=conv0.bias.detach(), stats_mode=1 if train else 0)
        bn = self._bn(bn0, st0, n * h * w, train)
        logits, _ = ops.conv_fused([Seg(h0, ksize=1, scale=bn[0], shift=bn[1], relu=True)],
                                   I[('head', 4)], conv3.out_channels, bias=conv3.bias.detach())
        if self._nbt:
            torch._foreach_add_(self._nbt, 1)
        self._nbt = []
        rows, dlogits = ops.cross_entropy(logits, codes.reshape(-1), conv3.out_channels, want_grad)
        if tape is not None:
            tape.update(layers=layers, codes=codes, label=label, x_h=x_h, h0=h0, bn0=bn, dlogits=dlogits)
        return rows.mean(), logits, dlogits

    # ---- backward -----------------------------------------------------------------------------------------------
    def _layer_backward(self, L, r, g_v: Optional[Tensor], g_h: Tensor, need_dx: bool, I, li, label=None):
        """g_v / g_h: gradients w.r.t. this layer's (out_v, x_h').  Returns gradients w.r.t. (x_v, x_h); fills the
        layer's embedding gradient from the gates' per-image input-gradient sums."""
        dt = self.dtype
        c = L.hidden_size
        conv_r, bn_rm = L.horiz_resid[0], L.horiz_resid[1]
        sc_r, _, mean_r, rstd_r = r['bn_r']
        d_r = ops.code_bn_bwd(g_h, None, r['r'], sc_r, mean_r, rstd_r, self._grad(bn_rm.weight), self._grad(bn_rm.bias))
        d_out_h, _ = self._conv1x1_bwd(conv_r, Seg(r['out_h'], ksize=1), d_r, wt=I[(li, 'r')])
        emb = L.class_cond_embedding.weight.detach()
        sc, sh, mean, rstd = r['bn_h']
        ds, dsum_h = ops.cpx_gated_bwd(r['s'], emb, label, sc, sh, mean, rstd, d_out_h, self._grad(L.gate_h.bn.weight),
                                       self._grad(L.gate_h.bn.bias))
        c2 = 2 * c
        ops.wgrad(Seg(r['h_vert'], ksize=1), ds, c2, c2, self._grad(L.vert_to_horiz.weight), bias_grad=self._grad(L.vert_to_horiz.bias),
                  bias_grad2=self._grad(L.horiz_stack.bias))
        k2 = L.kernel // 2
        in_h = r['in_h']
        cin_h = in_h.x.shape[-1]
        gh = self._grad(L.horiz_stack.weight)
        if L.kernel == 3:
            ops.wgrad(in_h, ds, c2, cin_h, gh, taps=(3, 2))
        else:
            gwh = torch.empty((c2, cin_h, in_h.ksize, in_h.ksize), dtype=torch.float32, device=ds.device)
            ops.wgrad(in_h, ds, c2, cin_h, gwh)
            self._post.append(lambda: gh.copy_(gwh.reshape(c2, 1, k2 + 1, c).permute(0, 3, 1, 2)))
        # gate_v (the last layer's out_v feeds nothing: no gradient for its BatchNorm, only ds_h reaches the embedding)
        d_hv, dsum_v = None, None
        if g_v is not None:
            sc, sh, mean, rstd = r['bn_v']
            d_hv, dsum_v = ops.cpx_gated_bwd(r['h_vert'], emb, label, sc, sh, mean, rstd, g_v, self._grad(L.gate_v.bn.weight),
                                             self._grad(L.gate_v.bn.bias))
        ops.cpx_embed_bwd(dsum_v, dsum_h, label, self._grad(L.class_cond_embedding.weight))
        d_hv, _ = ops.conv_fused([Seg(ds, ksize=1)], I[(li, 'v2h')], c2, res=d_hv)
        in_v = r['in_v']
        cin_v = in_v.x.shape[-1]
        gv = self._grad(L.vert_stack.weight)
        if L.kernel == 3:
            ops.wgrad(in_v, d_hv, c2, cin_v, gv, bias_grad=self._grad(L.vert_stack.bias), taps=(0, 6))
        else:
            gwv = torch.empty((c2, cin_v, in_v.ksize, in_v.ksize), dtype=torch.float32, device=ds.device)
            ops.wgrad(in_v, d_hv, c2, cin_v, gwv, bias_grad=self._grad(L.vert_stack.bias))
            self._post.append(lambda: gv.copy_(gwv.reshape(c2, k2 + 1, L.kernel, c).permute(0, 3, 1, 2)))
        if not need_dx:
            return None, None
        res_h = g_h if L.residual else None
        if L.kernel == 3:
            d_xh, _ = ops.conv_fused([Seg(ds)], I[(li, 'h')], c, res=res_h)
            d_xv, _ = ops.conv_fused([Seg(d_hv)], I[(li, 'v')], c)
        else:
            dcol_h, _ = ops.conv_fused([Seg(ds, ksize=1)], ops.prep_weight(_t1x1(r['wh']), dt), r['wh'].shape[1])
            d_xh = ops.col2im(dcol_h, c, 1, k2 + 1, 0, k2)
            if res_h is not None:
                d_xh = d_xh + res_h
            dcol_v, _ = ops.conv_fused([Seg(d_hv, ksize=1)], ops.prep_weight(_t1x1(r['wv']), dt), r['wv'].shape[1])
            d_xv = ops.col2im(dcol_v, c, k2 + 1, L.kernel, k2, k2)
        return d_xv, d_xh

    def _backward_body(self, tape):
        m = self.m
        oc = m.output_conv
        conv0, bn0, conv3 = oc[0], oc[1], oc[3]
        sc, sh, mean, rstd = tape['bn0']
        h0 = tape['h0']
        I = self._images(True)
        dz, st = self._conv1x1_bwd(conv3, Seg(h0, ksize=1, scale=sc, shift=sh, relu=True), tape['dlogits'], wt=I[('head', 4)],
                                   gate_x=h0, gscale=sc, gshift=sh, gmean=mean, grstd=rstd, stats_mode=2)
        n, h, w, _ = h0.shape
        d_h0 = ops.bn_backward(st, dz, h0, n * h * w, sc, mean, rstd, self._grad(bn0.weight), self._grad(bn0.bias))
        g_h, _ = self._conv1x1_bwd(conv0, Seg(tape['x_h'], ksize=1), d_h0, wt=I[('head', 0)])
        g_v = None                                              # the last layer's out_v feeds nothing
        layers, label = tape['layers'], tape['label']
        for i in reversed(range(len(m.layers))):
            g_v, g_h = self._layer_backward(m.layers[i], layers[i], g_v, g_h, True, I, i, label)
        d_x = g_v + g_h                                          # layer 0: x_v and x_h are the same embedding output
        # the code embedding's gradient in a fixed order (no index_add_, whose float atomics would make replays differ)
        ops.cpx_code_embed_bwd(d_x, tape['codes'], self._grad(m.embedding.weight))
