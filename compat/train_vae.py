#!/usr/bin/env python3
"""Driver counterpart of the reference's src/train_vae.py for the MI355X path: same CLI (train_vae.py:18-28), same
hard overrides (:29-36: pivot BCE, metrics Loss + BCE, Adam 3e-4, ReduceLROnPlateau), same experiment structure and loop
body (:38-148) -- see compat/_single.py for the shared parts and for what differs from the reference and why.
--model_name mcvae or cvae (the conditional baseline, models/cvae.py; with --control_name None, on one GPU)."""
import _single
from _single import cfg, Driver, parse


class VAEDriver(Driver):
    from mcgen_amd.trainer import VAETrainer as trainer_cls

    def fused_capture(self, input):
        self.tr.capture(input['img'], input['label'])

    def fused_step(self, input):                      # train_vae.py:106-111 as one replayed step
        return self.tr.train_iteration(input['img'], input['label'])


MODELS = ('mcvae', 'cvae')


def apply_control():
    """train_vae.py:24-27: --control_name None gives the baseline an empty control (tag <seed>_<data>_<subset>_cvae); any
    other control name keeps the MC form parse() gave it."""
    if cfg.get('control_name') == 'None':
        cfg['control'], cfg['control_name'] = {}, ''


def main():
    extra = parse({'pivot_metric': 'BCE', 'metric_name': {'train': ['Loss', 'BCE'], 'test': ['Loss', 'BCE']}, 'show': False})
    apply_control()
    if cfg['model_name'] not in MODELS:
        raise ValueError('Not valid model name')
    if cfg['model_name'] == 'cvae' and int(cfg['world_size']) > 1:
        raise ValueError('CVAE training runs on one GPU: multi-GPU CVAE is not supported; run with --world_size 1')
    VAEDriver(extra).main()


if __name__ == '__main__':
    main()
