"""Parameter initialisation, spectral-norm applicator and codebook / label-embedding surgery with the reference's
names and arity (src/models/utils.py:7-152); the plumbing every fused model shares (engine holder, autograd bridge)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from ..config import cfg
from ..modules import sample_codebook


def compute_dtype() -> torch.dtype:
    return {'float32': torch.float32, 'bfloat16': torch.bfloat16}[cfg.get('compute_dtype', 'float32')]


class FusedNet(nn.Module):
    """A module computed by a fused engine: the lazily built engine and the compute dtype switch."""
    _engine_cls = None

    def _engine(self):
        eng = self.__dict__.get('_eng')
        if eng is None or eng.dtype != self.compute_dtype:
            eng = self._engine_cls(self, self.compute_dtype)
            self.__dict__['_eng'] = eng
        return eng

    @property
    def compute_dtype(self):
        return self.__dict__.get('_cdt') or compute_dtype()

    def set_compute_dtype(self, dtype):
        self.__dict__['_cdt'] = dtype
        return self

    def _loss_node(self, run, holder: dict):
        """The training loss as one autograd node over every trainable parameter (see EngineLossFn)."""
        params = [p for p in self.parameters() if p.requires_grad]
        return EngineLossFn.apply(self._engine(), run, holder, *params)


class EngineLossFn(torch.autograd.Function):
    """One autograd node for a whole model: only the loss carries gradient.  `run(holder)` runs the engine's forward on a
    tape, may leave further outputs in `holder`, and returns (loss, backward): backward() replays the tape, its parameter
    gradients collected in the engine's gradient sink."""

    @staticmethod
    def forward(ctx, engine, run, holder, *params):
        loss, ctx.backward_fn = run(holder)
        ctx.engine, ctx.params = engine, params
        return loss

    @staticmethod
    def backward(ctx, gloss):
        eng = ctx.engine
        sink = {}
        eng._gsink = sink
        try:
            ctx.backward_fn()
        finally:
            eng._gsink = None
        ctx.backward_fn = None
        return (None, None, None) + tuple(sink[id(p)] * gloss if id(p) in sink else None for p in ctx.params)


def init_param(m):
    """models/utils.py:7-14: BN weight ~ N(1, 0.02), bias 0; xavier_uniform(gain 1) on
    Linear/Conv weights for the GAN models only."""
    if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0.0)
    if cfg['model_name'] in ['cgan', 'mcgan'] and isinstance(m, (nn.Linear, nn.Conv2d, nn.ConvTranspose2d)):
        nn.init.xavier_uniform_(m.weight.data, 1.)
    return m


def make_SpectralNormalization(m):
    """models/utils.py:17-21.  torch's own hook object is reused only as the CONTAINER of
    weight_orig / weight_u / weight_v (identical state_dict keys); the fused engine never calls
    the wrapped module's forward -- power iteration and W/sigma run in mcgen_sn_power_iter /
    mcgen_prep_weight."""
    if isinstance(m, (nn.Linear, nn.Conv2d, nn.ConvTranspose2d)):
        return torch.nn.utils.spectral_norm(m)
    return m


def live_modes(tables, built=None, train=False) -> int:
    """The mode count of label-embedding tables, read from the live weights at call time: `tables` = [(name, modes)] of every
    table a call will index.  create() swaps tables for ones with another number of modes, so nothing caches this count:
    the host-side label check and the gather kernels both take it from the same tensors.  Tables that disagree, or a
    training-mode call (`train`) on tables that no longer have the `built` count of the constructor, raise ValueError."""
    counts = {modes for _, modes in tables}
    if len(counts) != 1:
        raise ValueError('Not valid embedding: the label tables disagree about the number of modes: '
                         + ', '.join(f'{n} has {m}' for n, m in tables))
    modes = counts.pop()
    if train and built is not None and modes != built:
        raise ValueError(f'Not valid mode: the label tables hold {modes} modes but the model was built for {built}; '
                         'after create() only evaluation-mode generation is supported')
    return modes


def check_labels(label, modes: int):
    """int64 vector of labels in [0, modes), checked on the host before any launch (the reference's F.one_hot rejects
    the others; the gather kernels must never see one)."""
    if label.dtype != torch.int64 or label.dim() != 1:
        raise ValueError('Not valid label: expected an int64 vector of class indices')
    if label.numel() and (int(label.min()) < 0 or int(label.max()) >= modes):
        raise ValueError(f'Not valid label: every label must lie in [0, {modes})')
    return label


def _is_mc(module) -> bool:
    return module.__class__.__name__ == 'MultimodalController'


def create_codebook(codebook):
    """New distinct Bernoulli(0.5) codes for cfg['classes_size'] modes (models/utils.py:34-44)."""
    return sample_codebook(cfg['classes_size'], codebook.size(1), 0.5).to(cfg['device'])


def create_embedding(embedding):
    """Dirichlet(1) convex combinations of the existing embedding rows, one per new mode (models/utils.py:24-31):
    embedding [modes, E] -> [cfg['classes_size'], E]."""
    c = embedding.size(0)
    mix = torch.distributions.dirichlet.Dirichlet(torch.ones(c, device=embedding.device)).sample((cfg['classes_size'],))
    return mix.matmul(embedding).to(cfg['device'])


def _embedding_table(model, name, module):
    """How the reference's create / transit address `module` as a label-embedding table of `model`
    (models/utils.py:54-56, 64-66, 74-75, 84-86): (to_rows, from_rows) between the weight and its [modes, E] form, or None
    when the module is not one.  The dispatch is the reference's: by the model's class name, the module's type and the depth
    of its name."""
    cls, parts = model.__class__.__name__, name.split('.')
    columns = (lambda w: w.t()), (lambda rows: rows.t().contiguous())
    if 'VAE' in cls:
        return columns if isinstance(module, nn.Linear) and len(parts) == 2 and 'embedding' in parts[1] else None
    if 'PixelCNN' in cls:
        if isinstance(module, nn.Embedding) and len(parts) >= 3 and 'class_cond_embedding' in parts[2]:
            return (lambda w: w), (lambda rows: rows.contiguous())
        return None
    if 'Glow' in cls:
        if len(parts) == 4 and 'embedding' in parts[2]:
            return (lambda w: w.squeeze().t()), (lambda rows: rows.t().unsqueeze(2).unsqueeze(3).contiguous())
        return None
    if 'GAN' in cls:
        return columns if isinstance(module, nn.Linear) and len(parts) >= 2 and 'embedding' in parts[1] else None
    return None


def create(model):
    """New modes for cfg['classes_size'] labels (models/utils.py:47-88): every MultimodalController gets a fresh codebook,
    every label-embedding table of a c* baseline is replaced by Dirichlet mixtures of its rows -- a new nn.Parameter, as the
    reference installs it, whose mode count the models read from its shape at call time.  The tables are stored contiguous:
    the gather kernels index them as dense [E, modes] / [modes, 2C]."""
    for name, module in model.named_modules():
        if _is_mc(module):
            module.register_buffer('codebook', create_codebook(module.codebook))
            continue
        table = _embedding_table(model, name, module)
        if table is not None:
            to_rows, from_rows = table
            module.weight = nn.Parameter(from_rows(create_embedding(to_rows(module.weight))))
    return


def transit_codebook(codebook, root, alpha):
    """Splice the root mode's first round((1-alpha)*C) code bits into every other mode
    (models/utils.py:101-109)."""
    cb = codebook.detach().cpu().numpy()
    root_code = cb[root]
    others = np.delete(cb, root, 0)
    cross = int(round((1 - alpha) * cb.shape[1]))
    others[:, :cross] = root_code[:cross]
    return torch.tensor(np.insert(others, root, root_code, 0), device=cfg['device'])


def transit_embedding(embedding, root, alpha):
    """alpha * e_i + (1 - alpha) * e_root for every mode i, the root's row kept (models/utils.py:91-98)."""
    e = embedding.detach().cpu().numpy()
    alpha = float(alpha)          # a numpy float64 scalar (transit.py's np.linspace) would promote the float32 table to float64
    root_e = e[root]
    others = alpha * np.delete(e, root, 0) + (1 - alpha) * root_e
    return torch.tensor(np.insert(others, root, root_e, 0), device=cfg['device'])


def transit(model, root, alpha):
    """models/utils.py:112-152: keep the original codebook / embedding as `codebook_orig` / `weight_orig`, install the
    transited one as the live `codebook` / `weight`.  A spectral-normed embedding (CGAN's discriminator) already owns a
    `weight_orig`, which the reference reuses as the original.  The reference has no PixelCNN branch: MCPixelCNN's codebooks
    are spliced all the same, ConditionalGatedPixelCNN's tables stay."""
    pixelcnn = 'PixelCNN' in model.__class__.__name__
    for name, module in model.named_modules():
        if _is_mc(module):
            if not hasattr(module, 'codebook_orig'):
                module.register_buffer('codebook_orig', module.codebook.data)
            module.register_buffer('codebook', transit_codebook(module.codebook_orig, root, alpha))
            continue
        table = None if pixelcnn else _embedding_table(model, name, module)
        if table is not None:
            to_rows, from_rows = table
            if not hasattr(module, 'weight_orig'):
                module.register_buffer('weight_orig', module.weight.data)
            module.weight = nn.Parameter(from_rows(transit_embedding(to_rows(module.weight_orig), root, alpha)))
    return
