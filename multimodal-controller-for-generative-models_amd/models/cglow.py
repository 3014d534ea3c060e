"""CGlow, the reference's non-MC Glow baseline (src/models/cglow.py): MCGlow without any MultimodalController or Wrapper, where
the label enters through the prior of the last block: ``prior(zeros) + embedding(one_hot(label))``, ``embedding`` a 1x1
ZeroConv2d over the one-hot label that every Block owns and only the last one uses.

The module tree carries the reference's parameter / buffer names (``state_dict`` compatible, the three unused embeddings
included); the arithmetic runs in ``glow_engine.py`` (``CGlowEngine``) on HIP kernels.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..config import cfg
from ..glow_engine import CGlowEngine
from .mcglow import ActNorm, InvConv2dLU, MCGlow
from .utils import FusedNet, check_labels, init_param, live_modes


class ZeroConv2d(nn.Module):
    """cglow.py:119-130: zero-initialised conv whose output is multiplied by exp(3 * scale).  Not mcglow.py's class of the
    same name: that one is the 3x3 form only, as in the reference's mcglow.py, while the embedding here is 1x1 without padding
    and a reference user may pass the kernel geometry."""

    def __init__(self, input_size, output_size, kernel_size=3, stride=1, padding=1):
        super().__init__()
        self.conv = nn.Conv2d(input_size, output_size, kernel_size, stride, padding)
        self.conv.weight.data.zero_()
        self.conv.bias.data.zero_()
        self.scale = nn.Parameter(torch.zeros(1, output_size, 1, 1))


class AffineCoupling(nn.Module):
    """cglow.py:133-173 (affine form): Conv3 -> ActNorm -> ReLU -> Conv1 -> ActNorm -> ReLU -> ZeroConv2d."""

    def __init__(self, input_size, hidden_size=512, affine=True):
        super().__init__()
        if not affine:
            raise ValueError('Not valid coupling: only the affine form (cfg glow.affine = True) is built')
        self.affine = affine
        self.net = nn.Sequential(
            nn.Conv2d(input_size // 2, hidden_size, 3, padding=1), ActNorm(hidden_size, logdet=False), nn.ReLU(inplace=True),
            nn.Conv2d(hidden_size, hidden_size, 1), ActNorm(hidden_size, logdet=False), nn.ReLU(inplace=True),
            ZeroConv2d(hidden_size, input_size))
        for conv in (self.net[0], self.net[3]):
            conv.weight.data.normal_(0, 0.05)
            conv.bias.data.zero_()


class Flow(nn.Module):
    """cglow.py:176-199."""

    def __init__(self, input_size, hidden_size, affine=True, conv_lu=True):
        super().__init__()
        if not conv_lu:
            raise ValueError('Not valid invertible conv: only the LU form (cfg glow.conv_lu = True) is built')
        self.actnorm = ActNorm(input_size)
        self.invconv = InvConv2dLU(input_size)
        self.coupling = AffineCoupling(input_size, hidden_size, affine=affine)


class Block(nn.Module):
    """cglow.py:202-267: squeeze, K flows, split prior (or the label-conditioned prior of the last block); ``embedding`` is
    built in every block and read by the last one only."""

    def __init__(self, input_size, hidden_size, K, split=True, affine=True, conv_lu=True, num_mode=None):
        super().__init__()
        self.flows = nn.ModuleList(Flow(input_size * 4, hidden_size, affine=affine, conv_lu=conv_lu) for _ in range(K))
        self.split = split
        self.prior = ZeroConv2d(input_size * 2, input_size * 4) if split else ZeroConv2d(input_size * 4, input_size * 8)
        self.embedding = ZeroConv2d(num_mode, input_size * 8, 1, 1, 0)


class CGlow(FusedNet):
    """cglow.py:270-351."""
    _engine_cls = CGlowEngine

    def __init__(self, data_shape, hidden_size, K, L, affine=True, conv_lu=True, num_mode=None):
        super().__init__()
        self.data_shape, self.K, self.L, self.num_mode = data_shape, K, L, num_mode
        self.blocks = nn.ModuleList()
        c = data_shape[0]
        for _ in range(L - 1):
            self.blocks.append(Block(c, hidden_size, K, True, affine, conv_lu, num_mode))
            c *= 2
        self.blocks.append(Block(c, hidden_size, K, False, affine, conv_lu, num_mode))

    def _label(self, label):
        """The prior kernel gives a label outside the table a zero embedding row; the reference's F.one_hot (cglow.py:298,317)
        rejects one, so it is refused here, on the host, before any launch.
        The bound is the column count of the live table the prior kernel gathers from: the last block's."""
        tables = [(f'blocks.{len(self.blocks) - 1}.embedding.conv', self.blocks[-1].embedding.conv.weight.shape[1])]
        return check_labels(label, live_modes(tables, self.num_mode, self.training))

    def forward(self, input):
        """Negative log-likelihood in bits/dim (cglow.py:284-313).  The dequantisation noise U(0,1)/256 is drawn here unless
        `input['noise']` supplies it (parity runs)."""
        label = self._label(input['label'])
        noise = input['noise'] if 'noise' in input else torch.rand_like(input['img'])
        if torch.is_grad_enabled() and self.training:
            img, eng = input['img'], self._engine()

            def run(holder):
                tape = []
                loss, holder['z'] = eng.forward(img, None, noise, True, tape, label=label)
                return loss, lambda: eng.backward(tape, img.shape[0], float(img[0].numel()))

            holder = {}
            loss = self._loss_node(run, holder)
            return {'loss': loss, 'z': holder['z']}
        loss, z = self._engine().forward(input['img'], None, noise, self.training, label=label)
        return {'loss': loss, 'z': z}

    def reverse(self, input):
        return {'img': self._engine().reverse(input['z'], None, bool(input['reconstruct']), label=self._label(input['label']))}

    make_z_shapes = MCGlow.make_z_shapes

    def generate(self, C, x=None, temperature=1):
        if x is None:
            x = [torch.randn([C.size(0), *s], device=cfg['device']) * temperature for s in self.make_z_shapes()]
        return self.reverse({'z': x, 'reconstruct': False, 'label': C})['img']


def cglow():
    g = cfg['glow']
    model = CGlow(cfg['data_shape'], g['hidden_size'], g['K'], g['L'], g['affine'], g['conv_lu'], cfg['classes_size'])
    model.apply(init_param)
    return model
