"""Incremental eval-mode ancestral sampling of MCGatedPixelCNN on csrc/pixelcnn_sample.hip.

MCGatedPixelCNN.generate (mcpixelcnn.py:103-112) runs one full forward per position.  In eval mode BatchNorm is a
per-channel affine and every MultimodalController row belongs to one sample, so each pixel of each layer depends only on
positions already drawn and is final once they are:
  - vertical stack, row i: layer 0 reads the embedded codes of rows i-3 .. i-1 (the 4x7 mask-A kernel without its last
    row), layer l >= 1 reads out_v of layer l-1 at rows i-1 .. i; gate_v and vert_to_horiz follow pixel by pixel;
  - horizontal stack, (i, j): layer 0 reads the embedded codes of row i, columns j-3 .. j-1 (the 1x4 kernel without its
    last column), layer l >= 1 reads x_h of layer l-1 at columns j-1 .. j, plus vert_to_horiz at (i, j); gate_h,
    horiz_resid, the residual and the head follow.
So one call issues H row launches and H*W column launches back to back: every pixel of every layer is computed once (the
arithmetic of ONE full forward), with no host synchronisation and no torch work between the launches.
ConditionalGatedPixelCNN (models/cpixelcnn.py) runs the same schedule on the conditional kernel forms: the per-sample rows of
every layer's class_cond_embedding are added to both gate inputs, and no controller multiplies anything."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib, ops
from .engine_base import _unwrap

Tensor = torch.Tensor


def _r16(x: int) -> int:
    return (x + 15) // 16 * 16


def _r32(x: int) -> int:
    return (x + 31) // 32 * 32


def _mat(w: Tensor, rows: int, k: int) -> Tensor:
    """[R, K] -> zero-padded [rows, k] (the kernels' [Nout][Kp] weight images, K contiguous)."""
    w = w.reshape(w.shape[0], -1)
    return F.pad(w, (0, k - w.shape[1], 0, rows - w.shape[0]))


def conditional(m) -> bool:
    """ConditionalGatedPixelCNN (label embedding rows) rather than MCGatedPixelCNN (MultimodalController codes)."""
    return hasattr(m.layers[0], 'class_cond_embedding')


def num_modes(m) -> int:
    if conditional(m):
        from .models.cpixelcnn import table_modes
        return table_modes(m)            # the live tables' rows: create() replaces them
    return m.output_conv[3].codebook.shape[0]


def controllers(m):
    """Every MultimodalController in the order the kernels read their code rows (the engine's CodeBatch order)."""
    return [mc for L in m.layers for mc in (L.gate_v.mc, L.gate_h.mc, L.horiz_resid[2])] + [m.output_conv[3]]


def pack(m, dtype: torch.dtype):
    """-> (embedding [Kq, C] in `dtype`, weight pack in `dtype`, fp32 pack) in the layout of csrc/pixelcnn_sample.hip."""
    c, n_layer = m.hidden_size, len(m.layers)
    oc = m.output_conv
    conv0, bn0, conv4 = _unwrap(oc[0]), _unwrap(oc[1]), _unwrap(oc[-1])
    hd, kq = conv0.out_channels, conv4.out_channels
    if c % 8 or hd % 8 or m.layers[0].kernel != 7 or any(L.kernel != 3 for L in m.layers[1:]):
        raise ValueError('Not valid model for sample: a 7x7 first layer, 3x3 layers after it, channels a multiple of 8')
    mats, vecs = [], []
    for li, L in enumerate(m.layers):
        if L.mask_type == 'A':
            L.make_causal()                                   # zeroes the parameters in place, as the engine does
        wv, wh = L.vert_stack.weight.detach(), L.horiz_stack.weight.detach()
        if li == 0:
            wv, wh = wv[:, :, :3], wh[:, :, :, :3]            # the live taps of the mask-A kernels
        vm = wv.permute(0, 2, 3, 1).reshape(2 * c, -1)        # k = (tap row * KW + tap col) * C + channel
        hm = wh.permute(0, 2, 3, 1).reshape(2 * c, -1)
        mats += [_mat(vm, 2 * c, _r32(vm.shape[1])), _mat(L.vert_to_horiz.weight.detach(), 2 * c, _r32(2 * c)),
                 _mat(hm, 2 * c, _r32(hm.shape[1])), _mat(_unwrap(L.horiz_resid[0]).weight.detach(), _r16(c), _r32(c))]
        vecs += [L.vert_stack.bias, L.vert_to_horiz.bias, L.horiz_stack.bias, _unwrap(L.horiz_resid[0]).bias]
        for bn in (L.gate_v.bn, L.gate_h.bn, _unwrap(L.horiz_resid[1])):
            vecs += list(ops.bn_eval_affine(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps))
    mats += [_mat(conv0.weight.detach(), _r16(hd), _r32(c)), _mat(conv4.weight.detach(), _r16(kq), _r32(hd))]
    vecs += [conv0.bias, *ops.bn_eval_affine(bn0.weight.detach(), bn0.bias.detach(), bn0.running_mean, bn0.running_var, bn0.eps),
             conv4.bias]
    w = torch.cat([x.reshape(-1) for x in mats]).to(dtype).contiguous()
    if w.numel() != _lib.load().mcgen_px_sample_weight_elems(c, n_layer, hd, kq):
        raise _lib.McgenError('pixelcnn sampler: weight pack does not match the kernel layout')
    p = torch.cat([v.detach().float().reshape(-1) for v in vecs]).contiguous()
    emb = m.embedding.weight.detach().to(dtype).contiguous()
    return emb, w, p


def _code_rows(codes) -> Tensor:
    """The CodeBatch views as one flat buffer ([L][3][N][C] + [N][Hd]); they already are one when laid end to end."""
    base, off = codes[0].data_ptr(), 0
    for cd in codes:
        if cd.data_ptr() != base + off * 4 or not cd.is_contiguous():
            return torch.cat([x.reshape(-1) for x in codes])
        off += cd.numel()
    return codes[0].view(-1).as_strided((off,), (1,))


def validate(m, label: Tensor):
    """The checks `sample` makes before any launch."""
    if m.training:
        raise ValueError('Not valid mode: sample needs eval mode (batch-statistics BatchNorm makes the incremental form inexact)')
    if label.dtype != torch.int64:
        raise ValueError(f'Not valid label dtype: {label.dtype}, sample needs int64')
    modes = num_modes(m)
    if label.numel() and (int(label.min()) < 0 or int(label.max()) >= modes):
        raise ValueError(f'Not valid label: every label must lie in [0, {modes})')


def sample(m, label: Tensor, x: Tensor, dtype: torch.dtype, uniform: Optional[Tensor] = None, greedy: bool = False,
           return_logits: bool = False):
    """Fill the int64 code map x [N, H, W] in place, position by position in raster order; -> (x, logits [N, Kq, H, W] or
    None).  uniform [H*W, N] fp32 drives the inverse-CDF draw (ignored when greedy)."""
    n, h, w = x.shape
    c, n_layer = m.hidden_size, len(m.layers)
    hd, kq = _unwrap(m.output_conv[0]).out_channels, _unwrap(m.output_conv[-1]).out_channels
    if x.dtype != torch.int64 or not x.is_contiguous() or label.shape != (n,):
        raise ValueError('Not valid input: x must be a contiguous int64 [N, H, W] map and the label [N]')
    dev = x.device
    if uniform is None:
        uniform = torch.rand((h * w, n), device=dev) if not greedy else torch.zeros((h * w, n), device=dev)
    if uniform.dtype != torch.float32 or tuple(uniform.shape) != (h * w, n):
        raise ValueError(f'Not valid uniform: fp32 [{h * w}, {n}] expected')
    uniform = uniform.contiguous()
    emb, wpack, ppack = pack(m, dtype)
    cond = conditional(m)
    if cond:                                    # [L][N][2C]: every layer's embedding row of every sample, one launch
        mc = ops.cpx_gather_rows(torch.stack([L.class_cond_embedding.weight.detach() for L in m.layers]), label)
    else:
        mc = _code_rows(ops.CodeBatch(controllers(m)).run_labels(label))
    ov = torch.empty((n_layer, n, 2, w, c), dtype=dtype, device=dev)
    v2h = torch.empty((n_layer, n, w, 2 * c), dtype=torch.float32, device=dev)
    xh = torch.empty((n_layer, n, w, c), dtype=dtype, device=dev)
    logits = torch.empty((n, h, w, kq), dtype=torch.float32, device=dev) if return_logits else None
    P = _lib.PxSample()
    P.codes, P.emb, P.w, P.p, P.mc = ops._p(x), ops._p(emb), ops._p(wpack), ops._f32(ppack), ops._f32(mc)
    P.ov, P.v2h, P.xh, P.uniform, P.logits = ops._p(ov), ops._f32(v2h), ops._p(xh), ops._f32(uniform), ops._f32(logits)
    P.N, P.H, P.W, P.C, P.L, P.Kq, P.Hd, P.greedy = n, h, w, c, n_layer, kq, hd, int(greedy)
    row, col = (ops.cpx_sample_row, ops.cpx_sample_col) if cond else (ops.px_sample_row, ops.px_sample_col)
    for i in range(h):
        row(P, i, dtype)
        for j in range(w):
            col(P, i, j, dtype)
    # every buffer the launches read stays referenced until here; the stream orders their later reuse
    del emb, wpack, ppack, mc, ov, v2h, xh, uniform
    return x, (logits.permute(0, 3, 1, 2).contiguous() if logits is not None else None)
