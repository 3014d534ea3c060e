"""ConditionalGatedPixelCNN, the reference's non-MC PixelCNN baseline (src/models/cpixelcnn.py): MCGatedPixelCNN without any
MultimodalController or Wrapper, where every layer instead adds a per-label embedding row (class_cond_embedding, 2C wide)
to both gate inputs.  The module tree carries the reference's parameter / buffer names (``state_dict`` compatible); the
arithmetic runs in ``cpixelcnn_engine.py`` on HIP kernels."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..config import cfg
from ..cpixelcnn_engine import CPixelCNNEngine
from .utils import FusedNet, init_param, live_modes


def _check_labels(m, label):
    """Labels are gathered on the device with no host check inside the kernels (they clamp): refuse bad ones up front."""
    if label.dtype != torch.int64:
        raise ValueError(f'Not valid label dtype: {label.dtype}, CPixelCNN needs int64')
    modes = table_modes(m)
    if label.numel() and (int(label.min()) < 0 or int(label.max()) >= modes):
        raise ValueError(f'Not valid label: every label must lie in [0, {modes})')


def table_modes(m) -> int:
    """The row count of the live class_cond_embedding tables (every layer gathers from its own, so all must agree); a
    training-mode model whose tables no longer have the constructor's count is refused."""
    tables = [(f'layers.{i}.class_cond_embedding', L.class_cond_embedding.weight.shape[0]) for i, L in enumerate(m.layers)]
    return live_modes(tables, m.layers[0].class_cond_embedding.num_embeddings, m.training)


class GatedActivation(nn.Module):
    """cpixelcnn.py:8-18 -- parameter container of one gate: ``bn`` over the first half of the 2C input (the arithmetic,
    with the layer's embedding row added to the input, is mcgen_cpx_gated_fwd / the gate backward)."""

    def __init__(self, hidden_size):
        super().__init__()
        self.bn, self.activation = nn.BatchNorm2d(hidden_size), nn.ReLU(inplace=True)


class ConditionalGatedMaskedConv2d(nn.Module):
    """cpixelcnn.py:21-62 -- one gated layer: the MCGatedMaskedConv2d stacks and links, a class_cond_embedding
    [num_mode, 2C] whose row is added to h_vert before gate_v and to vert_to_horiz(h_vert) + horiz_stack(x_h) before
    gate_h, and a plain 1x1 -> BN residual branch."""

    def __init__(self, mask_type, hidden_size, kernel, residual, num_mode):
        super().__init__()
        if kernel % 2 != 1:
            raise ValueError('Not valid kernel size: must be odd')
        self.mask_type, self.residual, self.kernel, self.hidden_size = mask_type, residual, kernel, hidden_size
        half, c, c2 = kernel // 2, hidden_size, 2 * hidden_size
        self.class_cond_embedding = nn.Embedding(num_mode, c2)
        self.vert_stack = nn.Conv2d(c, c2, kernel_size=(half + 1, kernel), stride=1, padding=(half, half))
        self.vert_to_horiz = nn.Conv2d(c2, c2, kernel_size=1)
        self.horiz_stack = nn.Conv2d(c, c2, kernel_size=(1, half + 1), stride=1, padding=(0, half))
        self.gate_v, self.gate_h = GatedActivation(c), GatedActivation(c)
        self.horiz_resid = nn.Sequential(nn.Conv2d(c, c, kernel_size=1), nn.BatchNorm2d(c))

    def make_causal(self):
        """Mask 'A' (cpixelcnn.py:42-44): zeroes the parameters in place, on every forward of the first layer."""
        with torch.no_grad():
            self.vert_stack.weight[:, :, -1].zero_()
            self.horiz_stack.weight[:, :, :, -1].zero_()


class ConditionalGatedPixelCNN(FusedNet):
    """cpixelcnn.py:65-108 -- embedding of the code map, one 7x7 mask-A layer without residual, 3x3 mask-B layers with
    residual, a two-layer 1x1 head over 512 channels."""
    _engine_cls = CPixelCNNEngine

    def __init__(self, input_size=256, hidden_size=64, num_layer=15, num_mode=10):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        self.embedding = nn.Embedding(input_size, hidden_size)
        first = ConditionalGatedMaskedConv2d('A', hidden_size, 7, False, num_mode)
        rest = [ConditionalGatedMaskedConv2d('B', hidden_size, 3, True, num_mode) for _ in range(num_layer - 1)]
        self.layers = nn.ModuleList([first] + rest)
        head = 512
        self.output_conv = nn.Sequential(nn.Conv2d(hidden_size, head, 1), nn.BatchNorm2d(head), nn.ReLU(True),
                                         nn.Conv2d(head, input_size, 1))

    def forward(self, input):
        """{'img': int64 code map [N,H,W], 'label': int64 [N] in [0, num_mode)} -> {'logits' [N,K,H,W] fp32, 'loss'}
        (cpixelcnn.py:86-98)."""
        codes, label = input['img'], input['label']
        if codes.dtype != torch.int64:
            raise ValueError('Not valid input: the code map must be int64')
        _check_labels(self, label)
        eng = self._engine()
        if torch.is_grad_enabled() and self.training:

            def run(holder):
                tape = {}
                loss, holder['logits'], _ = eng.forward(codes, label, True, tape, want_grad=True)
                return loss, lambda: eng.backward(tape)

            holder = {}
            loss = self._loss_node(run, holder)
            logits = holder['logits']
        else:
            loss, logits, _ = eng.forward(codes, label, self.training)
        from .. import ops
        return {'loss': loss, 'logits': ops.to_nchw(logits, self.input_size)}

    def generate(self, C, x=None, sampler=None):
        """Ancestral sampling, one full forward per position (cpixelcnn.py:100-108).  `sampler(probs [N, K]) -> [N]`
        replaces the multinomial draw (parity tests decode greedily; the reference's call is the default)."""
        if x is None:
            x = torch.zeros((C.size(0), 8, 8), dtype=torch.long, device=cfg['device'])
        if sampler is None:
            sampler = lambda p: p.multinomial(1).squeeze(-1)                  # noqa: E731
        inp = {'img': x, 'label': C}
        with torch.no_grad():
            for i in range(x.size(1)):
                for j in range(x.size(2)):
                    out = self.forward(inp)
                    probs = F.softmax(out['logits'][:, :, i, j], -1)
                    inp['img'][:, i, j].copy_(sampler(probs))
        return inp['img']

    def sample(self, C, x=None, uniform=None, greedy=False, return_logits=False):
        """Eval-mode ancestral sampling with the contract of MCGatedPixelCNN.sample (pixelcnn_sampler.py): every pixel of
        every layer computed once; x [N, H, W] int64 (zeros [N, 8, 8] by default) is overwritten in place and returned.
        uniform [H*W, N] fp32 drives the inverse-CDF draw; greedy takes the first argmax.  return_logits: -> (x, logits)."""
        from .. import pixelcnn_sampler
        pixelcnn_sampler.validate(self, C)
        if x is None:
            x = torch.zeros((C.size(0), 8, 8), dtype=torch.long, device=cfg['device'])
        with torch.no_grad():
            x, logits = pixelcnn_sampler.sample(self, C, x, self.compute_dtype, uniform=uniform, greedy=greedy,
                                                return_logits=return_logits)
        return (x, logits) if return_logits else x


def cpixelcnn():
    p = cfg['pixelcnn']
    model = ConditionalGatedPixelCNN(input_size=p['num_embedding'], hidden_size=p['hidden_size'], num_layer=p['num_layer'],
                                     num_mode=cfg['classes_size'])
    model.apply(init_param)
    return model
