"""CGAN with the reference's module surface (src/models/cgan.py), computed by the fused HIP engines in
``cgan_engine.py``.

The module tree (class names, constructor signatures, parameter / buffer keys) is the reference's, so a reference
``model_dict`` loads with ``strict=True`` and vice versa.  The children are parameter containers:
``Generator.forward`` / ``Discriminator.forward`` run the whole network as fused kernels, behind autograd bridges so that
the reference's loop body runs with ``torch.optim.Adam``.  Eval mode uses the BatchNorm running statistics and spectral
norm without a power iteration, as the reference's modules do.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from ..cgan_engine import CDiscriminatorEngine, CGeneratorEngine
from ..config import cfg
from .utils import FusedNet, init_param, live_modes, make_SpectralNormalization


class GenResBlock(nn.Module):
    """cgan.py:8-36 (the generator builds stride-2 blocks only, cgan.py:45-46)."""

    def __init__(self, input_size, output_size, stride):
        super().__init__()
        if stride != 2:
            raise ValueError('Not valid stride')
        self.conv = nn.Sequential(
            nn.BatchNorm2d(input_size), nn.ReLU(), nn.Upsample(scale_factor=stride, mode='nearest'),
            nn.Conv2d(input_size, output_size, 3, 1, 1),
            nn.BatchNorm2d(output_size), nn.ReLU(),
            nn.Conv2d(output_size, output_size, 3, 1, 1))
        self.shortcut = nn.Sequential(nn.Upsample(scale_factor=stride, mode='nearest'), nn.Conv2d(input_size, output_size, 1, 1, 0))


class _GenFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, z, label, train, *params):
        img, saved = eng.forward(z, None, train, label=label)
        ctx.eng, ctx.saved = eng, saved
        return img

    @staticmethod
    def backward(ctx, dimg):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError('gradient w.r.t. the latent z is not produced by the fused generator')
        eng = ctx.eng
        gflat = torch.empty_like(eng.flat_p.flat)
        eng.backward(ctx.saved, dimg.contiguous(), gflat, accumulate=False)
        return (None, None, None, None, *eng.flat_p.views(gflat))


class Generator(FusedNet):
    _engine_cls = CGeneratorEngine

    def __init__(self, data_shape, latent_size, hidden_size, num_mode, embedding_size):
        super().__init__()
        self.latent_size = latent_size
        self.embedding = nn.Linear(num_mode, embedding_size, bias=False)
        self.linear = nn.Linear(latent_size + embedding_size, hidden_size[0] * 4 * 4)
        blocks = [GenResBlock(a, b, 2) for a, b in zip(hidden_size[:-1], hidden_size[1:])]
        blocks += [nn.BatchNorm2d(hidden_size[-1]), nn.ReLU(), nn.Conv2d(hidden_size[-1], data_shape[0], 3, 1, 1), nn.Tanh()]
        self.blocks = nn.Sequential(*blocks)

    def table_modes(self, train: bool) -> int:
        """The column count of the live embedding table, the one the engine gathers from."""
        w = self.embedding.weight
        return live_modes([('generator.embedding', w.shape[1])], self.embedding.in_features, train)

    def forward(self, input, indicator, label: Optional[torch.Tensor] = None):
        """cgan.py:55-62.  The embedding is a column gather W[:, label]: `label` (int64) when the caller has it, else the
        argmax of the one-hot `indicator`."""
        eng = self._engine()
        eng.rebind()
        eng.flat_p.ensure()
        lab = label if label is not None else indicator.argmax(1)
        return _GenFn.apply(eng, input, lab, self.training, *eng.flat_p.tensors)


class DisResBlock(nn.Module):
    """cgan.py:65-97: stride 2 pools both branches; stride 1 keeps an identity shortcut unless the channel count changes."""

    def __init__(self, input_size, output_size, stride):
        super().__init__()
        main = [nn.ReLU(), nn.Conv2d(input_size, output_size, 3, 1, 1), nn.ReLU(), nn.Conv2d(output_size, output_size, 3, 1, 1)]
        side = []
        if stride > 1 or input_size != output_size:
            side = [nn.Conv2d(input_size, output_size, 1, 1, 0)]
        if stride > 1:
            main.append(nn.AvgPool2d(2, stride=stride, padding=0))
            side.append(nn.AvgPool2d(2, stride=stride, padding=0))
        self.conv = nn.Sequential(*main)
        self.shortcut = nn.Sequential(*side)


class FirstDisResBlock(nn.Module):
    """cgan.py:100-120."""

    def __init__(self, input_size, output_size):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(input_size, output_size, 3, 1, 1), nn.ReLU(),
                                  nn.Conv2d(output_size, output_size, 3, 1, 1), nn.AvgPool2d(2))
        self.shortcut = nn.Sequential(nn.Conv2d(input_size, output_size, 1, 1, 0), nn.AvgPool2d(2))


class GlobalSumPooling(nn.Module):
    def forward(self, input):          # cgan.py:123-129; container only, the tail kernel does the sum
        return input.sum(dim=[-2, -1]).view(input.size(0), -1)


class _DisFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, x, label, train, *params):
        logit, saved = eng.forward(x, None, train, label=label)
        ctx.eng, ctx.saved = eng, saved
        return logit

    @staticmethod
    def backward(ctx, dlogit):
        eng = ctx.eng
        want_w = any(ctx.needs_input_grad[4:])
        gflat = torch.empty_like(eng.flat_p.flat) if want_w else None
        dimg = eng.backward(ctx.saved, dlogit.contiguous().view(-1), gflat, accumulate=False,
                            need_input_grad=ctx.needs_input_grad[1])
        grads = eng.flat_p.views(gflat) if want_w else [None] * len(eng.flat_p.tensors)
        return (None, dimg, None, None, *grads)


class Discriminator(FusedNet):
    _engine_cls = CDiscriminatorEngine

    def __init__(self, data_shape, hidden_size, num_mode, embedding_size):
        super().__init__()
        self.data_shape = data_shape
        h = hidden_size
        self.embedding = nn.Linear(num_mode, embedding_size, bias=False)
        blocks = [FirstDisResBlock(data_shape[0] + embedding_size, h[0])]
        # cgan.py:137-153: CIFAR10 keeps two stride-1 blocks at 8x8, the other datasets one
        n_down = len(h) - 3 if cfg['data_name'] in ['CIFAR10'] else len(h) - 2
        for i in range(len(h) - 1):
            blocks.append(DisResBlock(h[i], h[i + 1], stride=2 if i < n_down else 1))
        blocks += [nn.ReLU(), GlobalSumPooling(), nn.Linear(h[-1], 1)]
        self.blocks = nn.Sequential(*blocks)

    def table_modes(self, train: bool) -> int:
        """The column count of the table the engine gathers from: the spectral norm's `weight_orig`.  create() / transit()
        install a `weight` parameter beside it that the engine (like the reference's own spectral-norm hook) cannot use,
        after create() with another width than `weight_orig`: the discriminator is refused from then on."""
        emb = self.embedding
        if 'weight' in emb._parameters:
            raise ValueError('Not valid discriminator: create() / transit() replaced discriminator.embedding.weight '
                             f'({tuple(emb.weight.shape)}) while the spectral norm keeps weight_orig '
                             f'({tuple(emb.weight_orig.shape)}); only the generator runs after surgery')
        return live_modes([('discriminator.embedding', emb.weight_orig.shape[1])], emb.in_features, train)

    def forward(self, input, indicator, label: Optional[torch.Tensor] = None):
        """cgan.py:164-170 (`label` as in Generator.forward)."""
        self.table_modes(self.training)
        eng = self._engine()
        eng._ensure_flat()
        lab = label if label is not None else indicator.argmax(1)
        return _DisFn.apply(eng, input, lab, self.training, *eng.flat_p.tensors)


class CGAN(nn.Module):
    """cgan.py:173-200."""
    label_embedding = True          # GANTrainer: labels go to the engines, there are no MultimodalController codes

    def __init__(self, data_shape, latent_size, generator_hidden_size, discriminator_hidden_size, num_mode, embedding_size):
        super().__init__()
        self.latent_size = latent_size
        self.generator = Generator(data_shape, latent_size, generator_hidden_size, num_mode, embedding_size)
        self.discriminator = Discriminator(data_shape, discriminator_hidden_size, num_mode, embedding_size)
        self.discriminator.apply(make_SpectralNormalization)

    def set_compute_dtype(self, dtype):
        self.generator.set_compute_dtype(dtype)
        self.discriminator.set_compute_dtype(dtype)
        return self

    def _labels(self, C, net):
        """The engines gather embedding columns by label, so the one-hot indicator of the reference (cgan.py:183,188) is
        not built.  Its F.one_hot rejects a label outside the table: evaluation mode checks that here (one host read)
        against the column count of the live table `net`'s engine gathers from, and raises ValueError before any launch;
        training mode adds no host synchronisation -- there the kernels give such a label a zero embedding and no
        gradient, and never read outside the embedding."""
        if C.dtype != torch.int64 or C.dim() != 1:
            raise ValueError(f'labels must be a 1-d int64 tensor, got {C.dtype} {tuple(C.shape)}')
        modes = net.table_modes(self.training)
        if not self.training and C.numel() and not (0 <= int(C.min()) and int(C.max()) < modes):
            raise ValueError(f'labels must lie in [0, {modes})')
        return C

    def generate(self, C, x=None):
        C = self._labels(C, self.generator)
        if x is None:
            x = torch.randn([C.size(0), self.latent_size], device=cfg['device'])
        return self.generator(x, None, label=C)

    def discriminate(self, x, C):
        return self.discriminator(x, None, label=self._labels(C, self.discriminator))

    def forward(self, input):
        x = torch.randn(input['img'].size(0), self.latent_size, device=cfg['device'])
        return self.discriminate(self.generate(input['label'], x), input['label'])


def cgan():
    """Zero-argument factory reading cfg, as models/cgan.py:203-213."""
    model = CGAN(cfg['data_shape'], cfg['gan']['latent_size'], cfg['gan']['generator_hidden_size'],
                 cfg['gan']['discriminator_hidden_size'], cfg['classes_size'], cfg['gan']['embedding_size'])
    model.apply(init_param)
    return model
