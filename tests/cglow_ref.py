"""Float64 restatement of CGlow's label-conditioned prior (reference: models/cglow.py, Block.forward of the last block) and of
its parameter gradients, written from the formulas alone, plus the fixture plumbing the CGlow tests share.

prior = ZeroConv2d(c, 2c, 3, 1, 1) on zeros, embedding = ZeroConv2d(M, 2c, 1, 1, 0) on the one-hot label,
ZeroConv2d(x) = (conv(x) + b) * exp(3 * scale):

    h[n, co] = b_p[co] exp(3 s_p[co]) + (W_e[co, label_n] + b_e[co]) exp(3 s_e[co])        (every pixel)

A label outside [0, M) reads a zero embedding row and contributes no table gradient (the kernels' contract).
"""
from __future__ import annotations

import os

import numpy as np
import torch

import golden_util as gu


def prior(b_p, s_p, w_e, b_e, s_e, label, hw: int):
    """-> h [N, hw, C2] float64.  b_p, s_p, b_e, s_e [C2]; w_e [C2, M]; label [N] integers."""
    b_p, s_p, w_e, b_e, s_e = (np.asarray(t, dtype=np.float64) for t in (b_p, s_p, w_e, b_e, s_e))
    label = np.asarray(label)
    c2, m = w_e.shape
    ok = (label >= 0) & (label < m)
    emb = np.where(ok[:, None], w_e[:, np.where(ok, label, 0)].T, 0.0)                    # [N, C2]
    h = b_p * np.exp(3 * s_p) + (emb + b_e) * np.exp(3 * s_e)
    return np.repeat(h[:, None, :], hw, axis=1)


def prior_bwd(dprior, b_p, s_p, w_e, b_e, s_e, label):
    """dprior [N, hw, C2] -> dict of float64 gradients: b_p, s_p, w_e, b_e, s_e (prior.conv.weight's is zero)."""
    dprior, b_p, s_p, w_e, b_e, s_e = (np.asarray(t, dtype=np.float64) for t in (dprior, b_p, s_p, w_e, b_e, s_e))
    label = np.asarray(label)
    c2, m = w_e.shape
    dh = dprior.sum(1)                                                                    # [N, C2]
    rp, re = np.exp(3 * s_p), np.exp(3 * s_e)
    ok = (label >= 0) & (label < m)
    emb = np.where(ok[:, None], w_e[:, np.where(ok, label, 0)].T, 0.0)
    dw_e = np.zeros_like(w_e)
    for n in np.nonzero(ok)[0]:
        dw_e[:, label[n]] += dh[n] * re
    return {'b_p': dh.sum(0) * rp, 's_p': 3 * dh.sum(0) * b_p * rp, 'b_e': dh.sum(0) * re,
            's_e': 3 * (dh * (emb + b_e)).sum(0) * re, 'w_e': dw_e}


# ---- fixtures (tools/gen_golden.py: _cglow_small) ---------------------------------------------------------------------------
FIXTURES = [('cglow_small.npz', 12, 1), ('cglow_cifar_small.npz', 10, 3), ('cglow_omniglot_small.npz', 1623, 1)]
GLOW_CFG = {'hidden_size': 32, 'K': 2, 'L': 3, 'affine': True, 'conv_lu': True}
_CACHE = {}


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
