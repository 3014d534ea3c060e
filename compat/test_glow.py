#!/usr/bin/env python3
"""Driver counterpart of the reference's src/test_glow.py:40-82: the trained MCGlow / CGlow over the train loader in eval mode,
metric Loss (:26), the trailing n = 1 append (:73), the 'test' line, then the last batch through `model.reverse` with
reconstruct=True and that batch's z (:77-79) for the input_ / output_ grids (:80-81), and output/result/<model_tag>.pt.
Shared parts: compat/_evaluate.py."""
from _evaluate import EvalDriver


class GlowTest(EvalDriver):
    metric_names = ['Loss']
    grids = True

    def reconstruct(self, model, input, output):          # test_glow.py:77-79
        input['reconstruct'] = True
        input['z'] = output['z']
        return model.reverse(input)


if __name__ == '__main__':
    GlowTest().main(('mcglow', 'cglow'))
