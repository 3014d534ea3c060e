#!/usr/bin/env python3
"""Driver counterpart of the reference's src/train_glow.py for the MI355X path: train_vae.py's structure plus the
data-dependent ActNorm initialisation on `num_init_batches` (8) concatenated batches BEFORE the resume / data-parallel
wrap (train_glow.py:37,60-67) and the reconstruction through `model.reverse` in test() (:156-158).  Shared parts and
the differences from the reference: compat/_single.py.
--model_name mcglow or cglow (the conditional baseline, models/cglow.py; with --control_name None, on one GPU).
--glow_affine {True,False} / --glow_conv_lu {True,False} pick MCGlow's coupling form and 1x1 convolution (compat/_flags.py:
applied to cfg['glow'] after process_control; default: the table's True, True; a False is refused for cglow)."""
from itertools import islice

import torch

import _single
from _flags import apply_glow_flags, pop_glow_flags
from _single import cfg, Driver, parse, to_device


class GlowDriver(Driver):
    from mcgen_amd.trainer import GlowTrainer as trainer_cls
    glow_flags = {}                                   # --glow_affine / --glow_conv_lu, popped in main()

    def after_control(self):
        apply_glow_flags(cfg, self.glow_flags)

    def before_resume(self, model, loader):           # train_glow.py:60-67
        batches = list(islice(loader, None, cfg['num_init_batches']))
        init = {k: torch.cat([b[k] for b in batches], 0) for k in ('img', 'label')}
        with torch.no_grad():
            model.train(True)
            model(to_device(init, cfg['device']))

    def fused_capture(self, input):
        self.tr.capture(input['img'], input['label'])

    def fused_step(self, input):
        return self.tr.train_iteration(input['img'], input['label'])

    def test_output(self, model, input):              # train_glow.py:153-158
        output = model(input)
        input['reconstruct'] = True
        input['z'] = output['z']
        rec = model.reverse(input)
        return dict(output, **{k: v for k, v in rec.items() if k not in output}) if isinstance(rec, dict) else output


MODELS = ('mcglow', 'cglow')


def apply_control():
    """train_glow.py:24-27: --control_name None gives the baseline an empty control (tag <seed>_<data>_<subset>_cglow); any
    other control name keeps the MC form parse() gave it."""
    if cfg.get('control_name') == 'None':
        cfg['control'], cfg['control_name'] = {}, ''


def main():
    GlowDriver.glow_flags = pop_glow_flags()
    extra = parse({'pivot_metric': 'Loss', 'metric_name': {'train': ['Loss'], 'test': ['Loss']}, 'show': False,
                   'num_init_batches': 8})
    apply_control()
    if cfg['model_name'] not in MODELS:
        raise ValueError('Not valid model name')
    if cfg['model_name'] == 'cglow' and int(cfg['world_size']) > 1:
        raise ValueError('CGlow training runs on one GPU: multi-GPU CGlow is not supported; run with --world_size 1')
    GlowDriver(extra).main()


if __name__ == '__main__':
    main()
