#!/usr/bin/env python3
"""Driver counterpart of the reference's src/test_vae.py:40-78: the trained MCVAE / CVAE (<model_tag>_best.pt) over the train
loader in eval mode, metrics Loss + BCE (:26), the last batch appended once more with n = 1 (:72), the 'test' line, the grids
output/vis/input_<tag> / output_<tag> of the last batch's first 100 images (:76-77) and output/result/<model_tag>.pt.
Shared parts and the --metrics device / host switch: compat/_evaluate.py."""
from _evaluate import EvalDriver


class VAETest(EvalDriver):
    metric_names = ['Loss', 'BCE']
    grids = True


if __name__ == '__main__':
    VAETest().main(('mcvae', 'cvae'))
