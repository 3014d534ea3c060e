"""Float64 restatement of the MCGlow training likelihood for every combination of coupling form (affine / additive) and 1x1
convolution (LU / plain InvConv2d), written from the formulas of the reference's models/mcglow.py alone, plus the fixture
plumbing the variant tests share.  oracle/ knows only affine + LU; this file covers the other three.

Per flow on x [N, C, H, W] (mcglow.py:188-195):
    ActNorm      y = scale * (x + loc)                      logdet += H W sum log|scale|
    InvConv2d    y = W x  (1x1)                             logdet += H W log|det W|          (plain: W is the parameter;
                 LU: W = P (L o l_mask + I) (U o u_mask + diag(s_sign exp(w_s))), log|det W| = sum w_s)
    coupling     h = net(y_a); affine: y_b <- (y_b + t) s, s = sigmoid(log_s + 2), [log_s | t] = h, logdet_n += sum log s
                               additive: y_b <- y_b + h     (no log-determinant)
net = Conv3x3 -> ActNorm -> ReLU -> code -> Conv1x1 -> ActNorm -> ReLU -> code -> ZeroConv2d, code = codebook[label],
ZeroConv2d(x) = (conv3x3(x) + b) * exp(3 scale).  Blocks squeeze 2x2 into channels, run K flows and split off half of the
channels under a Gaussian prior ZeroConv2d(kept half) (the last block: all channels, prior ZeroConv2d(zeros)).
loss = mean_n -( -log(256) D + logdet_n + logp_n ) / (log(2) D), D = C H W of the image (mcglow.py:283-293).
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import golden_util as gu

# (fixture, classes, channels, affine, conv_lu): tools/gen_golden.py::_mcglow_variant_small
FIXTURES = [('mcglow_additive_small.npz', 12, 1, False, True),
            ('mcglow_plainconv_small.npz', 12, 1, True, False),
            ('mcglow_plain_additive_cifar_small.npz', 10, 3, False, False)]
K, L, HIDDEN = 2, 3, 32
_CACHE = {}


def glow_cfg(affine, conv_lu):
    return {'hidden_size': HIDDEN, 'K': K, 'L': L, 'affine': affine, 'conv_lu': conv_lu}


def load(name):
    """The fixture, with its `_step` companion file (first-step gradients, final differences) merged in where it has one;
    loaded once per session and shared."""
    if name not in _CACHE:
        d = gu.load_npz(name)
        step = name.replace('.npz', '_step.npz')
        if os.path.exists(gu.golden_path(step)):
            d.update(gu.load_npz(step))
        _CACHE[name] = d
    return _CACHE[name]


def layout(d):
    """The reference's state_dict layout the fixture recorded: {key: shape}, in state_dict order."""
    out = {}
    for s in d['layout']:
        k, dims = str(s).rsplit(':', 1)
        out[k] = tuple(int(x) for x in dims.split('x')) if dims else ()
    return out


def states(d):
    """(start, after the ActNorm initialisation, after the training steps) as state dicts in the layout's order."""
    sd0 = gu.state_from_npz(d, 'sd/')
    sd0 = {k: sd0[k] for k in layout(d)}
    init = dict(sd0, **gu.state_from_npz(d, 'sd_init/'))
    final = {k: (v + torch.from_numpy(d['sd_final_delta/' + k]) if 'sd_final_delta/' + k in d else v) for k, v in init.items()}
    return sd0, init, final


# ---- float64 likelihood ---------------------------------------------------------------------------------------------------
def _zero_conv(p, pre, x):
    return (F.conv2d(x, p[pre + 'conv.weight'], p[pre + 'conv.bias'], padding=1)) * torch.exp(3 * p[pre + 'scale'])


def _squeeze(x):
    n, c, h, w = x.shape
    return x.view(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(n, c * 4, h // 2, w // 2)


def _logp(x, mean, log_sd):
    return (-0.5 * math.log(2 * math.pi) - log_sd - 0.5 * (x - mean) ** 2 / torch.exp(2 * log_sd)).flatten(1).sum(1)


def invconv_matrix(p, pre):
    """(W, log|det W|) of the flow's 1x1 convolution from the parameters under `pre` ('....invconv.')."""
    if pre + 'weight' in p:
        w = p[pre + 'weight'][:, :, 0, 0]
        return w, torch.linalg.slogdet(w)[1]
    c = p[pre + 'w_s'].numel()
    u_mask = torch.triu(torch.ones(c, c, dtype=torch.float64), 1)
    w = p[pre + 'w_p'] @ (p[pre + 'w_l'] * u_mask.T + torch.eye(c, dtype=torch.float64)) @ \
        (p[pre + 'w_u'] * u_mask + torch.diag(p[pre + 's_sign'] * torch.exp(p[pre + 'w_s'])))
    return w, p[pre + 'w_s'].sum()


def nll(p, img, label, noise):
    """Training-mode bits/dim of initialised weights `p` (a dict of float64 tensors; those that need gradients are leaves
    with requires_grad) for img [N, C, H, W], int64 labels and the dequantisation noise."""
    x = img.double() * 0.5 + noise.double() / 256
    n, d = x.shape[0], float(x[0].numel())
    logdet = torch.zeros(n, dtype=torch.float64)
    logp = torch.zeros(n, dtype=torch.float64)
    blocks = 1 + max(int(k.split('.')[1]) for k in p)
    for b in range(blocks):
        x = _squeeze(x)
        c, hw = x.shape[1], x.shape[2] * x.shape[3]
        f = 0
        while f'blocks.{b}.flows.{f}.actnorm.loc' in p:
            pre = f'blocks.{b}.flows.{f}.'
            x = p[pre + 'actnorm.scale'] * (x + p[pre + 'actnorm.loc'])
            w, lad = invconv_matrix(p, pre + 'invconv.')
            x = F.conv2d(x, w[:, :, None, None])
            logdet = logdet + hw * (torch.log(torch.abs(p[pre + 'actnorm.scale'])).sum() + lad)
            xa, xb = x.chunk(2, 1)
            net = pre + 'coupling.net.'
            h = F.conv2d(xa, p[net + '0.module.weight'], p[net + '0.module.bias'], padding=1)
            h = torch.relu(p[net + '1.module.scale'] * (h + p[net + '1.module.loc'])) * p[net + '3.codebook'][label][:, :, None, None]
            h = F.conv2d(h, p[net + '4.module.weight'], p[net + '4.module.bias'])
            h = torch.relu(p[net + '5.module.scale'] * (h + p[net + '5.module.loc'])) * p[net + '7.codebook'][label][:, :, None, None]
            h = _zero_conv(p, net + '8.module.', h)
            if h.shape[1] == c:                               # affine
                log_s, t = h.chunk(2, 1)
                s = torch.sigmoid(log_s + 2)
                xb = (xb + t) * s
                logdet = logdet + torch.log(s).flatten(1).sum(1)
            else:                                             # additive: c / 2 channels, no log-determinant
                assert h.shape[1] == c // 2
                xb = xb + h
            x = torch.cat([xa, xb], 1)
            f += 1
        pre = f'blocks.{b}.prior.'
        if b < blocks - 1:
            x, z = x.chunk(2, 1)
            mean, log_sd = _zero_conv(p, pre, x).chunk(2, 1)
            logp = logp + _logp(z, mean, log_sd)
        else:
            mean, log_sd = _zero_conv(p, pre, torch.zeros_like(x)).chunk(2, 1)
            logp = logp + _logp(x, mean, log_sd)
    loss = -(-math.log(256.) * d + logdet + logp) / (math.log(2.) * d)
    return loss.mean()


def loss_and_grads(init, img, label, noise, wanted):
    """(loss, {key: gradient}) in float64 for the parameter keys `wanted` of the initialised state `init`."""
    p = {k: v.double() for k, v in init.items() if v.dtype.is_floating_point}
    for k in wanted:
        p[k] = p[k].clone().requires_grad_(True)
    loss = nll(p, img, label, noise)
    grads = torch.autograd.grad(loss, [p[k] for k in wanted])
    return float(loss.detach()), dict(zip(wanted, grads))
