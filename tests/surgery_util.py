"""What the create / transit tests and their fixture generator (tools/gen_golden.py: fx_surgery_*) share: the four baselines'
base weights -- the reference's trained state of each model's existing *_small fixture -- and the reading of the
surgery_<model>.npz fixtures, which carry only what the reference's create (10 -> 14 modes) and transit(root 2, alpha) change."""
from __future__ import annotations

import numpy as np
import torch

import cglow_ref
import golden_util as gu

BASE = {'cgan': 'cgan_small.npz', 'cvae': 'cvae_small.npz', 'cpixelcnn': 'cpixelcnn_small.npz', 'cglow': 'cglow_cifar_small.npz'}
MODES, NEW_MODES, ROOT, ALPHAS, CREATE_SEED = 10, 14, 2, (0.0, 0.5, 1.0), 20240
_CACHE = {}


def base_state(model: str):
    """The reference's state after the base fixture's training steps, as a state dict in the reference's key order."""
    if model not in _CACHE:
        d = cglow_ref.load(BASE[model])
        if model == 'cglow':
            sd = cglow_ref.states(d)[2]
        else:
            sd = {}
            init = gu.procedural_state_generic(cglow_ref.layout(d), seed=int(d['sd_seed']))
            for k in cglow_ref.layout(d):
                if 'sd_final_int/' + k in d:
                    sd[k] = torch.from_numpy(np.array(d['sd_final_int/' + k]))
                else:
                    sd[k] = init[k] + torch.from_numpy(d['sd_delta/' + k].astype(np.float32))
        _CACHE[model] = sd
    return {k: v.clone() for k, v in _CACHE[model].items()}


def configure(model: str, device: str, cfg, classes: int = MODES):
    """The small widths of the base fixtures in `cfg` (the reference's cfg in the generator, mcgen_amd's in the tests)."""
    cfg.update(model_name=model, device=device, classes_size=classes, data_name='CIFAR10', data_shape=[3, 32, 32])
    cfg['compute_dtype'] = 'float32'
    if model == 'cgan':
        cfg['gan'] = {'latent_size': 128, 'generator_hidden_size': [32] * 4, 'discriminator_hidden_size': [16] * 4, 'embedding_size': 32}
    elif model == 'cvae':
        cfg['vae'] = {'hidden_size': [8, 16, 32], 'latent_size': 16, 'num_res_block': 2, 'embedding_size': 32}
    elif model == 'cpixelcnn':
        cfg['pixelcnn'] = {'num_layer': 4, 'hidden_size': 16, 'num_embedding': 32}
    else:
        cfg['glow'] = dict(cglow_ref.GLOW_CFG)


def inputs(model: str, modes: int, seed: int = 31):
    """(labels [B] reaching the last of `modes` modes, the root and a repeat; the latent x generate takes, or None for
    cpixelcnn, whose decode is greedy)."""
    g = torch.Generator().manual_seed(seed + modes)
    b = {'cgan': 8, 'cvae': 8, 'cglow': 4, 'cpixelcnn': 6}[model]
    label = torch.tensor([modes - 1, ROOT, 0, modes - 1, modes // 2, 1, modes - 2, 3][:b])
    if model == 'cgan':
        return label, torch.randn(b, 128, generator=g)
    if model == 'cvae':
        return label, torch.randn(b, 16, generator=g)
    if model == 'cglow':
        return label, [0.7 * torch.randn(b, *s, generator=g) for s in ((6, 16, 16), (12, 8, 8), (48, 4, 4))]
    return label, None


def changed(sd, base):
    """The entries of state dict `sd` that are new or differ from `base`."""
    return {k: v for k, v in sd.items() if k not in base or v.shape != base[k].shape or not torch.equal(v, base[k])}


def load(model: str):
    return cglow_ref.load(f'surgery_{model}.npz')


def fixture_state(model: str, d, tag: str):
    """The module-tree tensors the reference leaves after the surgery `tag` ('create', 'transit0' .. 'transit2'): the base
    state with the fixture's changed tensors, restricted to and ordered by the fixture's key list."""
    sd = base_state(model)
    for k in d:
        if k.startswith(tag + '/'):
            sd[k[len(tag) + 1:]] = torch.from_numpy(np.array(d[k]))
    return {k: sd[k] for k in d[tag.rstrip('012') + '_keys'].tolist()}
