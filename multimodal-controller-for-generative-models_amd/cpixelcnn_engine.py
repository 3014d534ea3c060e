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

from . import ops
from .pixelcnn_engine import PixelCNNEngine

Tensor = torch.Tensor


class CPixelCNNEngine(PixelCNNEngine):
    _CONV_GATE_STATS = False             # the gate statistics are those of the biased inputs (mcgen_cpx_gate_stats)

    def _gates_fwd(self, L, h_vert: Tensor, st_v, s: Tensor, st_s, label: Tensor, train: bool, count: int):
        """-> (out_v, out_h, bn_v, bn_h, None, None): gate(h_vert + e), gate(s + e) in one launch; the row is added in the
        kernel, so h_vert stays unbiased for vert_to_horiz."""
        emb = L.class_cond_embedding.weight.detach()
        bv, bh = L.gate_v.bn, L.gate_h.bn
        if train:
            # the statistics of the BIASED inputs (the conv epilogue's would be those of h_vert / s): one launch for both gates
            st_v, st_s = ops.cpx_gate_stats([(h_vert, emb, label), (s, emb, label)])
            bn_v, bn_h = self._bn_pair(bv, st_v, bh, st_s, count)
        else:
            bn_v = self._bn(bv, None, count, False)
            bn_h = self._bn(bh, None, count, False)
        out_v, out_h = ops.cpx_gated_fwd([(h_vert, emb, label, bn_v[0], bn_v[1]), (s, emb, label, bn_h[0], bn_h[1])])
        return out_v, out_h, bn_v, bn_h, None, None

    def _gate_bwd(self, L, gate, x: Tensor, bn, code, g: Optional[Tensor], label: Tensor, aux=None):
        """-> (gradient w.r.t. the gate's input, its per-image channel sums).  gate_v's call, which gets gate_h's sums as
        aux, also fills the layer's embedding gradient from both (the last layer's gate_v has no gradient: only gate_h's
        sums reach the embedding there)."""
        emb = L.class_cond_embedding.weight.detach()
        dx = dsum = None
        if g is not None:
            sc, sh, mean, rstd = bn
            dx, dsum = ops.cpx_gated_bwd(x, emb, label, sc, sh, mean, rstd, g, self._grad(gate.bn.weight), self._grad(gate.bn.bias))
        if gate is L.gate_v:
            ops.cpx_embed_bwd(dsum, aux, label, self._grad(L.class_cond_embedding.weight))
        return dx, dsum

    def _code_embed_bwd(self, d_x: Tensor, codes: Tensor):
        # a fixed order (no index_add_, whose float atomics would make replays differ)
        ops.cpx_code_embed_bwd(d_x, codes, self._grad(self.m.embedding.weight))
