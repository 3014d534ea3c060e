#!/usr/bin/env python3
"""Driver counterpart of the reference's src/create.py:38-146 (the paper's "creating new modes" experiment): resume
<model_tag>_best.pt (and, for the PixelCNN models, the VQ-VAE's <ae_tag>_best.pt), give the model new modes with
`models.utils.create` -- fresh MultimodalController codebooks, Dirichlet mixtures of the baselines' label embeddings --
and generate from them in eval mode, in chunks of sample_per_iter = 1000.
  --save_npy True:  classes_size x generate_per_mode samples to output/npy/created_<model_tag>.npy, scaled
                    (x + 1) / 2 * 255, plus (save_img) one grid of save_per_mode samples per mode (create.py:58-86);
  otherwise:        re-create with 10 / 50 / 100 modes and write one grid of save_per_mode samples per mode each
                    (create.py:122-145).  Glow on CIFAR10 draws 1000 per mode instead and fills each mode's column with
                    NaN-free samples first (create.py:88-121).
The PixelCNN models draw their code maps with `model.sample` and decode them with `ae.decode_code`, as compat/generate.py
does.  Grids go through compat/utils.save_img; --generate_per_mode N overrides the process_control table.  The command
line, model loading and experiment loop are shared with transit.py and test_created.py (`main` below)."""
import torch

import _single  # noqa: F401  (sys.path)
import models
import data as data_shim
from _single import cfg, parse
from data import fetch_dataset
from _flags import apply_glow_flags, check_use_ema, pop_glow_flags, pop_use_ema
from generate import SAMPLE_PER_ITER, _draw, _pop_flag
from utils import process_control, process_dataset, resume, save, save_img

AVOID_OVERFLOW = 1000                                     # create.py:90


def _draw_all(model, ae, C):
    return torch.cat([_draw(model, ae, c.to(cfg['device'])).cpu() for c in torch.split(C, SAMPLE_PER_ITER)])


def _recreate(model, modes):
    cfg['classes_size'] = modes
    models.utils.create(model)
    model = model.to(cfg['device'])
    model.train(False)
    return model


def _prefer_finite(created, modes, per_mode):
    """create.py:107-119: per mode its first `per_mode` NaN-free samples, topped up with others; -> [per_mode * modes, ...]
    with the modes along a grid row."""
    saved = []
    for j in range(modes):
        mine = created[j:created.size(0):modes]
        valid = torch.sum(torch.isnan(mine), dim=(1, 2, 3)) == 0
        keep = mine[valid][:per_mode]
        saved.append(torch.cat([keep, mine[~valid][:max(per_mode - keep.size(0), 0)]], dim=0))
    saved = torch.cat(saved)
    saved = saved.view(modes, -1, *saved.size()[1:]).transpose(0, 1)
    return saved.reshape(-1, *saved.size()[2:])


def create(model, ae=None):
    """create.py:55-146."""
    with torch.no_grad():
        if cfg['save_npy']:
            models.utils.create(model)
            model = model.to(cfg['device'])
            model.train(False)
            created = _draw_all(model, ae, torch.arange(cfg['classes_size']).repeat(cfg['generate_per_mode']))
            created = (created + 1) / 2 * 255
            save(created.numpy(), './output/npy/created_{}.npy'.format(cfg['model_tag']), mode='numpy')
            if cfg['save_img']:
                save_num_mode = min(100, cfg['classes_size'])
                saved = torch.cat([created[i:i + save_num_mode]
                                   for i in range(0, cfg['classes_size'] * cfg['save_per_mode'], cfg['classes_size'])])
                save_img(saved, './output/vis/created_{}.{}'.format(cfg['model_tag'], cfg['save_format']),
                         nrow=save_num_mode, range=(0, 255))
            return
        glow_cifar = 'glow' in cfg['model_name'] and cfg['data_name'] in ['CIFAR10']
        for save_num_mode in (10, 50, 100):
            model = _recreate(model, save_num_mode)
            if glow_cifar:
                created = _draw_all(model, None, torch.arange(save_num_mode).repeat(AVOID_OVERFLOW))
                created = _prefer_finite(created, save_num_mode, cfg['save_per_mode'])
            else:
                created = _draw_all(model, ae, torch.arange(save_num_mode).repeat(cfg['save_per_mode']))
            save_img(created, './output/vis/created_{}_{}.{}'.format(cfg['model_tag'], save_num_mode, cfg['save_format']),
                     nrow=save_num_mode, range=(-1, 1))


def load_models_with_epoch(extra):
    """create.py:38-50: seed, dataset (for classes_size), the model and -- for the PixelCNN models -- its VQ-VAE, each
    from its *_best.pt; -> (model, ae or None, dataset, the epoch `resume` read for the model: 1 without a checkpoint)."""
    seed = int(cfg['model_tag'].split('_')[0])
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    data_shim._SYNTHETIC['train'] = extra['synthetic_size']
    dataset = fetch_dataset(cfg['data_name'], cfg['subset'])
    process_dataset(dataset['train'])
    ae = None
    if 'pixelcnn' in cfg['model_name']:
        ae = eval('models.{}().to(cfg["device"])'.format(cfg['ae_name']))
        _, ae, _, _, _ = resume(ae, cfg['ae_tag'], load_tag='best')
        ae.train(False)
    model = eval('models.{}().to(cfg["device"])'.format(cfg['model_name']))
    last_epoch, model, _, _, _ = resume(model, cfg['model_tag'], load_tag='best')
    if extra.get('use_ema'):                              # the averaged generator of a checkpoint trained with --ema_decay
        from generate import overlay_ema
        overlay_ema(model, cfg['model_tag'])
    if cfg.get('compute_dtype') == 'bfloat16':
        for m in (model, ae):
            if m is not None and hasattr(m, 'set_compute_dtype'):
                m.set_compute_dtype(torch.bfloat16)
    return model, ae, dataset, last_epoch


def load_models(extra):
    """-> (model, ae or None, dataset): load_models_with_epoch without the epoch."""
    return load_models_with_epoch(extra)[:3]


def main(run_experiment, overrides=None, accepts_ema=False):
    """create.py:25-35, the loop every evaluation driver of the reference repeats: one `run_experiment(extra)` per seed.
    `accepts_ema`: the driver loads a model, so it takes --use_ema {True,False} (mcgan / cgan: sample the averaged generator)."""
    per_mode = _pop_flag('--generate_per_mode')
    glow_flags = pop_glow_flags()                         # --glow_affine / --glow_conv_lu (mcglow)
    use_ema = pop_use_ema() if accepts_ema else False
    extra = parse(overrides or {})
    check_use_ema(use_ema, cfg['model_name'])
    extra['use_ema'] = use_ema
    if cfg['control_name'] == 'None':                     # the baselines take no control (create.py:19-22)
        cfg['control'] = {}
        cfg['control_name'] = ''
    process_control()
    apply_glow_flags(cfg, glow_flags)
    if per_mode is not None:
        cfg['generate_per_mode'] = int(per_mode)
    if torch.cuda.is_available():
        cfg['device'] = 'cuda:0'
    seeds = list(range(cfg['init_seed'], cfg['init_seed'] + cfg['num_experiments']))
    for i in range(cfg['num_experiments']):
        tag = [str(seeds[i]), cfg['data_name'], cfg['subset'], cfg['model_name'], cfg['control_name']]
        cfg['model_tag'] = '_'.join([x for x in tag if x])
        ae_tag = [str(seeds[i]), cfg['data_name'], cfg['subset'], cfg['ae_name']]
        cfg['ae_tag'] = '_'.join([x for x in ae_tag if x])
        print('Experiment: {}'.format(cfg['model_tag']))
        run_experiment(extra)


def run_experiment(extra):
    model, ae, _ = load_models(extra)
    create(model, ae)


if __name__ == '__main__':
    main(run_experiment, accepts_ema=True)
