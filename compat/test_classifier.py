#!/usr/bin/env python3
"""Driver counterpart of the reference's src/test_classifier.py:40-77: the trained feature classifier of IS / FID over the train
loader in eval mode, metrics Loss + Accuracy (:26), the 'test' line and output/result/<model_tag>.pt.  Unlike its siblings the
reference has no trailing `logger.append(evaluation, 'test')` here (:72-76), so there is none.  Run with --control_name None, as
train_classifier.py.  Shared parts: compat/_evaluate.py."""
from _evaluate import EvalDriver


class ClassifierTest(EvalDriver):
    metric_names = ['Loss', 'Accuracy']
    trailing_append = False


if __name__ == '__main__':
    ClassifierTest().main(('classifier',))
