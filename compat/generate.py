#!/usr/bin/env python3
"""Driver counterpart of the reference's src/generate.py:40-107: resume <model_tag>_best.pt (and, for MCPixelCNN, the
VQ-VAE's <ae_tag>_best.pt), then generate classes_size x generate_per_mode samples in eval mode, in chunks of
sample_per_iter = 1000.  MCPixelCNN draws its code maps with `model.sample` (every pixel of every layer computed once,
pixelcnn_sampler.py) and decodes them with `ae.decode_code`; MCGAN / CGAN / MCVAE / CVAE / MCGlow / CGlow call
`model.generate`.
  --save_npy True:  output/npy/generated_<model_tag>.npy, scaled (x + 1) / 2 * 255, plus (save_img) one grid of
                    save_per_mode samples per mode (generate.py:60-84);
  otherwise:        grids of 10 / 50 / 100 modes x save_per_mode samples (generate.py:85-104).
Grids go through compat/utils.save_img (the image, and a .npy next to the requested path).  --generate_per_mode N overrides the
process_control table (applied after it), so a short run is possible.  --glow_affine / --glow_conv_lu {True,False} pick
MCGlow's coupling form and 1x1 convolution the same way (compat/_flags.py).  --use_ema True (mcgan / cgan) samples the
averaged generator of a checkpoint trained with --ema_decay.  Shared CLI parsing: compat/_single.parse."""
import torch

import _single  # noqa: F401  (sys.path)
import models
import data as data_shim
from _flags import apply_glow_flags, check_use_ema, pop_flag, pop_glow_flags, pop_use_ema
from _single import cfg, parse
from data import fetch_dataset
from utils import load, process_control, process_dataset, resume, save, save_img

SAMPLE_PER_ITER = 1000                                    # generate.py:57


def _pop_flag(name):
    """Remove `--name V` / `--name=V` from argv (a cfg key that only process_control creates); -> V or None."""
    return pop_flag(name)


def _draw(model, ae, C):
    """One chunk of labels -> images in (-1, 1) (generate.py:66-71)."""
    if ae is None:
        return model.generate(C)
    return ae.decode_code(model.sample(C))


def generate(model, ae=None):
    """generate.py:54-105."""
    with torch.no_grad():
        model.train(False)
        if cfg['save_npy']:
            C = torch.arange(cfg['classes_size']).repeat(cfg['generate_per_mode'])
            generated = torch.cat([_draw(model, ae, c.to(cfg['device'])).cpu() for c in torch.split(C, SAMPLE_PER_ITER)])
            generated = (generated + 1) / 2 * 255
            save(generated.numpy(), './output/npy/generated_{}.npy'.format(cfg['model_tag']), mode='numpy')
            if cfg['save_img']:
                save_num_mode = min(100, cfg['classes_size'])
                saved = torch.cat([generated[i:i + save_num_mode]
                                   for i in range(0, cfg['classes_size'] * cfg['save_per_mode'], cfg['classes_size'])])
                save_img(saved, './output/vis/generated_{}.{}'.format(cfg['model_tag'], cfg['save_format']),
                         nrow=save_num_mode, range=(0, 255))
        else:
            for most in (10, 50, 100):
                if most > cfg['classes_size']:
                    continue
                save_num_mode = min(most, cfg['classes_size'])
                C = torch.arange(save_num_mode).repeat(cfg['save_per_mode'])
                saved = torch.cat([_draw(model, ae, c.to(cfg['device'])).cpu() for c in torch.split(C, SAMPLE_PER_ITER)])
                save_img(saved, './output/vis/generated_{}_{}.{}'.format(cfg['model_tag'], save_num_mode, cfg['save_format']),
                         nrow=save_num_mode, range=(-1, 1))


def overlay_ema(model, model_tag, load_tag='best'):
    """--use_ema True: the checkpoint's averaged generator (its 'generator_ema', written by train_gan.py --ema_decay) laid
    over the generator that `resume` just loaded."""
    from mcgen_amd.checkpoint import overlay_averaged_generator
    path = './output/model/{}_{}.pt'.format(model_tag, load_tag)
    model.generator.load_state_dict(overlay_averaged_generator(model.generator.state_dict(), load(path)))


def run_experiment(extra):
    """generate.py:40-51."""
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
    _, model, _, _, _ = resume(model, cfg['model_tag'], load_tag='best')
    if extra.get('use_ema'):
        overlay_ema(model, cfg['model_tag'])
    if cfg.get('compute_dtype') == 'bfloat16':
        for m in (model, ae):
            if m is not None and hasattr(m, 'set_compute_dtype'):
                m.set_compute_dtype(torch.bfloat16)
    generate(model, ae)


def main():
    per_mode = _pop_flag('--generate_per_mode')
    glow_flags = pop_glow_flags()
    use_ema = pop_use_ema()
    extra = parse({})
    check_use_ema(use_ema, cfg['model_name'])
    extra['use_ema'] = use_ema
    if cfg['control_name'] == 'None':                     # the baselines take no control (generate.py:19-22)
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


if __name__ == '__main__':
    main()
