#!/usr/bin/env python3
"""Driver counterpart of the reference's src/train_classifier.py for the MI355X path: the feature network of IS / FID on
COIL100 / Omniglot (metrics.py:49-55,89-95).  The shared structure of compat/_single.py with the classifier overrides
(train_classifier.py:23-36): `--control_name None` gives an empty control, so the model tag is
<seed>_<data>_<subset>_classifier -- with seed 0 the basename metrics.py loads from ./metrics_tf/res/classifier/; pivot
Accuracy, MAXIMISED (pivot -inf); metrics Loss + Accuracy; Adam lr 1e-2 (config.yml's weight_decay 0); MultiStepLR
milestones [100], gamma 0.1; 200 epochs.  `test()` runs the train loader in eval mode (:78), as _single.Driver does.
Differences from the reference: those of compat/_single.py, and 200 epochs is the default of --num_epochs rather than a
hard override, so a short run can be asked for.  Multi-GPU classifier training (nn.DataParallel in the reference) is
refused."""
import _single
from _single import cfg, Driver, parse


class ClassifierDriver(Driver):
    from mcgen_amd.trainer import ClassifierTrainer as trainer_cls
    pivot_max = True

    def fused_capture(self, input):
        self.tr.capture(input['img'], input['label'])

    def fused_step(self, input):                      # train_classifier.py:106-110 as one replayed step
        # a short final batch runs the eager step at its own size (_FlatTrainer._dispatch, shared by all single-network trainers)
        return self.tr.train_iteration(input['img'], input['label'])


def configure():
    """train_classifier.py:18-36 -> the parsed cfg; returns the driver's extra options."""
    cfg['num_epochs'] = 200                           # train_classifier.py:36 (here the --num_epochs default)
    extra = parse({'pivot_metric': 'Accuracy', 'pivot': -float('inf'), 'lr': 1e-2, 'weight_decay': 0,
                   'metric_name': {'train': ['Loss', 'Accuracy'], 'test': ['Loss', 'Accuracy']},
                   'scheduler_name': 'MultiStepLR', 'milestones': [100], 'factor': 0.1})
    if cfg['control_name'] == 'None':                 # train_classifier.py:23-25
        cfg['control'] = {}
        cfg['control_name'] = ''
    if cfg['model_name'] != 'classifier':
        raise ValueError('Not valid model name')
    if int(cfg['world_size']) > 1:
        raise ValueError('Not valid world_size: multi-GPU classifier training is not supported')
    return extra


def main():
    ClassifierDriver(configure()).main()


if __name__ == '__main__':
    main()
