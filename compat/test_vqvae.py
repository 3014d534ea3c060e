#!/usr/bin/env python3
"""Driver counterpart of the reference's src/test_vqvae.py:40-78: the trained VQ-VAE over the train loader in eval mode, metrics
Loss + MSE (:26), the trailing n = 1 append (:73), the 'test' line, the input_ / output_ grids (:77-78) and
output/result/<model_tag>.pt.  Run with --control_name None, as train_vqvae.py.  Shared parts: compat/_evaluate.py."""
from _evaluate import EvalDriver


class VQVAETest(EvalDriver):
    metric_names = ['Loss', 'MSE']
    grids = True


if __name__ == '__main__':
    VQVAETest().main(('vqvae',))
