"""CVAE, the reference's non-MC VAE baseline (src/models/cvae.py): MCVAE without any MultimodalController or Wrapper, where a
label embedding (``nn.Linear(num_mode, E, bias=False)`` over the one-hot label, i.e. a column of its weight) is concatenated
to the encoder's input image and to the latent in front of the decoder's Linear.  The module tree carries the reference's
parameter / buffer names (``state_dict`` compatible); the arithmetic runs in ``cvae_engine.py`` on HIP kernels."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from ..config import cfg
from ..cvae_engine import CVAEEngine
from ..vae_engine import check_train_batch
from .utils import FusedNet, check_labels, init_param, live_modes


def _bn_relu(width):
    return [nn.BatchNorm2d(width), nn.ReLU(inplace=True)]


def _encoded_shape(data_shape, widths):
    shrink = 2 ** len(widths)
    return (widths[-1], data_shape[1] // shrink, data_shape[2] // shrink)


class ResBlock(nn.Module):
    """cvae.py:16-31 -- ``conv`` holds conv, BN, ReLU, conv, BN (indices 0..4); the skip + ReLU live in the fused tail kernel."""

    def __init__(self, hidden_size):
        super().__init__()
        w = hidden_size
        self.conv = nn.Sequential(nn.Conv2d(w, w, 3, 1, 1), *_bn_relu(w), nn.Conv2d(w, w, 3, 1, 1), nn.BatchNorm2d(w))
        self.activation = nn.ReLU(inplace=True)


class Encoder(nn.Module):
    """cvae.py:34-67 -- ``embedding`` [E, num_mode]; ``blocks``: len(hidden) strided stages (the first over C + E channels),
    then the residual blocks; ``mu`` / ``logvar`` heads."""

    def __init__(self, data_shape, hidden_size, latent_size, num_res_block, num_mode, embedding_size):
        super().__init__()
        self.embedding = nn.Linear(num_mode, embedding_size, bias=False)
        layers, width_in = [], data_shape[0] + embedding_size
        for width in hidden_size:
            layers += [nn.Conv2d(width_in, width, 4, 2, 1)] + _bn_relu(width)
            width_in = width
        layers += [ResBlock(width_in) for _ in range(num_res_block)]
        self.blocks = nn.Sequential(*layers)
        self.encoded_shape = _encoded_shape(data_shape, hidden_size)
        features = int(np.prod(self.encoded_shape))
        self.mu, self.logvar = nn.Linear(features, latent_size), nn.Linear(features, latent_size)


class Decoder(nn.Module):
    """cvae.py:70-99 -- ``embedding`` [E, num_mode]; ``linear``: Linear over latent + E, BatchNorm1d, ReLU; ``blocks``: residual
    blocks, transposed-conv stages up to the image, Sigmoid."""

    def __init__(self, data_shape, hidden_size, latent_size, num_res_block, num_mode, embedding_size):
        super().__init__()
        self.embedding = nn.Linear(num_mode, embedding_size, bias=False)
        self.encoded_shape = _encoded_shape(data_shape, hidden_size)
        features = int(np.prod(self.encoded_shape))
        self.linear = nn.Sequential(nn.Linear(latent_size + embedding_size, features), nn.BatchNorm1d(features), nn.ReLU(inplace=True))
        layers = [ResBlock(hidden_size[-1]) for _ in range(num_res_block)]
        for wide, narrow in zip(reversed(hidden_size[1:]), reversed(hidden_size[:-1])):
            layers += [nn.ConvTranspose2d(wide, narrow, 4, 2, 1)] + _bn_relu(narrow)
        layers += [nn.ConvTranspose2d(hidden_size[0], data_shape[0], 4, 2, 1), nn.Sigmoid()]
        self.blocks = nn.Sequential(*layers)


class CVAE(FusedNet):
    """cvae.py:102-142."""
    _engine_cls = CVAEEngine

    def __init__(self, data_shape=(3, 32, 32), hidden_size=(64, 128, 256), latent_size=128, num_res_block=2,
                 num_mode=None, embedding_size=32):
        super().__init__()
        self.data_shape, self.hidden_size, self.latent_size = data_shape, hidden_size, latent_size
        self.num_res_block, self.num_mode, self.embedding_size = num_res_block, num_mode, embedding_size
        self.encoder = Encoder(data_shape, hidden_size, latent_size, num_res_block, num_mode, embedding_size)
        self.decoder = Decoder(data_shape, hidden_size, latent_size, num_res_block, num_mode, embedding_size)

    def _label(self, label, encoder=True):
        """The kernels gather embedding columns by label and give a label outside the table a zero row; the reference's
        F.one_hot (cvae.py:126,135) rejects one, so it is refused here, on the host, before any launch.  The bound is the
        column count of the live tables this call gathers from (the decoder's, and the encoder's unless `encoder` is False)."""
        tables = [('decoder.embedding', self.decoder.embedding.weight.shape[1])]
        if encoder:
            tables.append(('encoder.embedding', self.encoder.embedding.weight.shape[1]))
        return check_labels(label, live_modes(tables, self.num_mode, self.training))

    def generate(self, C, z=None):
        """Decode of a latent under the labels C (cvae.py:123-129) -> images in (-1, 1)."""
        if z is None:
            z = torch.randn([C.size(0), self.latent_size], device=cfg['device'])
        from .. import ops
        eng = self._engine()
        with torch.no_grad():
            logits = eng.decode(eng.latent_rows(z, self._label(C, encoder=False)), self.training, None)
        return torch.sigmoid(ops.to_nchw(logits, self.data_shape[0])) * 2 - 1

    def forward(self, input):
        """{'img' in (-1,1), 'label'[, 'eps']} -> {'loss', 'mu', 'logvar', 'img'} (cvae.py:131-142); `eps` injects the
        reparameterisation noise (parity runs), otherwise it is drawn here.  Evaluation mode takes z = mu."""
        if self.training:
            check_train_batch(input['img'].shape[0])           # one sample: refused before any launch, as the reference does
        eng = self._engine()
        label = self._label(input['label'])
        eps = input.get('eps')
        if torch.is_grad_enabled() and self.training:
            if eps is None:
                eps = torch.randn(input['img'].shape[0], self.latent_size, device=input['img'].device)

            def run(holder):
                tape = []
                out = eng.forward(input['img'], label, True, eps, tape, want_grad=True)
                holder.update(out)
                return out['loss'], lambda: eng.backward(tape, label)

            holder = {}
            loss = self._loss_node(run, holder)
            return {'loss': loss, 'mu': holder['mu'], 'logvar': holder['logvar'], 'img': holder['img']}
        return eng.forward(input['img'], label, self.training, eps)


def cvae():
    v = cfg['vae']
    model = CVAE(data_shape=cfg['data_shape'], hidden_size=v['hidden_size'], latent_size=v['latent_size'],
                 num_res_block=v['num_res_block'], num_mode=cfg['classes_size'], embedding_size=v['embedding_size'])
    model.apply(init_param)
    return model
