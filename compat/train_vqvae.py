#!/usr/bin/env python3
"""Driver counterpart of the reference's src/train_vqvae.py for the MI355X path: train_vae.py's structure with the
VQ-VAE overrides (train_vqvae.py:29-36: pivot MSE, metrics Loss + MSE, Adam 3e-4, ReduceLROnPlateau, show False) and
its control handling (:25-28): `--control_name None` gives an empty control, so the model tag is
<seed>_<data>_<subset>_vqvae -- the `ae_tag` that compat/train_pixelcnn.py resumes (train_pixelcnn.py:44-45,58-59).
Shared parts and the differences from the reference: compat/_single.py.  Multi-GPU VQ-VAE training is refused
(VQVAETrainer): per-rank EMA statistics would drift the codebooks apart."""
import _single
from _single import cfg, Driver, parse


class VQVAEDriver(Driver):
    from mcgen_amd.trainer import VQVAETrainer as trainer_cls

    def fused_capture(self, input):
        self.tr.capture(input['img'])

    def fused_step(self, input):                      # train_vqvae.py:104-108 as one replayed step
        # a short final batch runs the eager step at its own size and the captured graph keeps its statics: the trainers'
        # shared dispatch (_FlatTrainer._dispatch) decides by shapes and refuses anything but another batch size
        return self.tr.train_iteration(input['img'])


def main():
    extra = parse({'pivot_metric': 'MSE', 'metric_name': {'train': ['Loss', 'MSE'], 'test': ['Loss', 'MSE']}, 'show': False})
    if cfg['control_name'] == 'None':                 # train_vqvae.py:25-28
        cfg['control'] = {}
        cfg['control_name'] = ''
    if cfg['model_name'] != 'vqvae':
        raise ValueError('Not valid model name')
    if int(cfg['world_size']) > 1:
        raise ValueError('Not valid world_size: multi-GPU VQ-VAE training is not supported')
    VQVAEDriver(extra).main()


if __name__ == '__main__':
    main()
