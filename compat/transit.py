#!/usr/bin/env python3
"""Driver counterpart of the reference's src/transit.py:37-82 (the paper's "transiting between modes" experiment): resume
<model_tag>_best.pt and, for 10 / 50 / 100 modes (those the dataset has), draw ONE latent per mode, then for each of
save_per_mode + 1 values of alpha in [0, 1] call `models.utils.transit(model, 0, alpha)` -- every mode's codebook /
label embedding moved towards mode 0's, alpha = 1 being the trained model -- and `model.generate(C, x)` on that same
latent.  One grid per mode count: output/vis/transited_<model_tag>_<modes>, a row per alpha.
For mcgan / cgan / mcvae / cvae / mcglow / cglow; the reference has no PixelCNN transit, so those names are refused."""
import numpy as np
import torch

import _single  # noqa: F401  (sys.path)
import models
from _single import cfg
from create import load_models, main
from utils import save_img

ROOT = 0                                                  # transit.py:52


def _latent(model, n):
    """transit.py:61-71."""
    if cfg['model_name'] in ['cvae', 'mcvae']:
        return torch.randn([n, cfg['vae']['latent_size']]).to(cfg['device'])
    if cfg['model_name'] in ['cgan', 'mcgan']:
        return torch.randn([n, cfg['gan']['latent_size']]).to(cfg['device'])
    return [torch.randn([n, *s], device=cfg['device']) for s in model.make_z_shapes()]


def transit(model):
    """transit.py:49-82."""
    with torch.no_grad():
        model.train(False)
        alphas = np.linspace(0, 1, cfg['save_per_mode'] + 1)
        for most in (10, 50, 100):
            if most > cfg['classes_size']:
                continue
            save_num_mode = min(most, cfg['classes_size'])
            C = torch.arange(save_num_mode).to(cfg['device'])
            x = _latent(model, C.size(0))
            transited = []
            for alpha in alphas:
                models.utils.transit(model, ROOT, alpha)
                model = model.to(cfg['device'])
                transited.append(model.generate(C, x).cpu())
            transited = torch.stack(transited, dim=0)
            transited = transited.view(-1, *transited.size()[2:])
            save_img(transited, './output/vis/transited_{}_{}.{}'.format(cfg['model_tag'], save_num_mode, cfg['save_format']),
                     nrow=save_num_mode, range=(-1, 1))


def run_experiment(extra):
    if cfg['model_name'] not in ['mcgan', 'cgan', 'mcvae', 'cvae', 'mcglow', 'cglow']:
        raise ValueError('Not valid model name')
    model, _, _ = load_models(extra)
    transit(model)


if __name__ == '__main__':
    main(run_experiment, accepts_ema=True)       # --use_ema: transit on the averaged generator (mcgan / cgan)
