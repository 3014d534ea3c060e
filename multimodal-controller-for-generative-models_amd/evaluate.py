"""Per-batch evaluation metrics that stay on the device: the running means a test loop needs (the reference's test_vae.py:60-75
and its siblings: `Metric.evaluate` per batch, `Logger.append(evaluation, 'test', n)`) without a host synchronisation per
metric and batch.

`compat/metrics.Metric` ends every metric in float(...) or .item().  `DeviceEvaluator.update` instead launches the reductions
of csrc/eval_ops.hip on the tensors the eval forward has just written -- float64 sums in a fixed order -- which leave the batch
value in `last[slot]` and add n * value to `acc[slot]`, two small float64 device arrays; `result()`, or `fetch()` for the means and the
last values together, is the one device-to-host copy.  The weighted mean is the one `Logger.append` folds: sum n_i v_i / sum n_i.  Whole-set metrics (InceptionScore, FID,
DBI) are not per-batch sums and keep their own path (mcgen_amd.metrics)."""
from __future__ import annotations

import torch

from . import _lib, ops

SUPPORTED = ('Loss', 'Loss_G', 'Loss_D', 'MSE', 'BCE', 'PSNR', 'NLL', 'Accuracy')
_SCALAR_KEY = {'Loss': 'loss', 'Loss_G': 'loss_G', 'Loss_D': 'loss_D'}
_IMG = ('MSE', 'BCE', 'PSNR')


def _tensor(x, what):
    if not torch.is_tensor(x):
        raise ValueError(f'Not valid input type: {what} must be a tensor, got {type(x).__name__}')
    if not x.is_cuda:
        raise ValueError(f'Not valid input: {what} is on {x.device}; the device evaluator has no CPU path')
    return x.detach()


class DeviceEvaluator:
    """Running means of the per-batch metrics `names` (a subset of SUPPORTED) on `device`.  `Metric`'s key look-ups:
    output['loss' / 'loss_G' / 'loss_D'], output['img'] against input['img'] (MSE, BCE, PSNR: one launch pair for all three),
    output['logits'] against input['img'] (NLL), output['label'] against input['label'] (Accuracy)."""

    def __init__(self, names, device):
        names = list(names)
        unknown = [n for n in names if n not in SUPPORTED]
        if unknown:
            raise ValueError('Not valid metric name: {}: the device evaluator sums per-batch metrics only, {}'.format(
                unknown, ', '.join(SUPPORTED)))
        if len(set(names)) != len(names):
            raise ValueError('Not valid metric name: {} repeats a name'.format(names))
        device = torch.device(device)
        if device.type != 'cuda':
            raise ValueError(f'Not valid device: {device}; the device evaluator has no CPU path')
        self.names = names
        self.slot = {name: i for i, name in enumerate(names)}
        slots = _lib.CONSTANTS['MCGEN_EVAL_SLOTS']
        self.state = torch.zeros(2, slots, dtype=torch.float64, device=device)      # one tensor: one copy fetches both rows
        self.acc, self.last = self.state[0], self.state[1]
        self.work = torch.empty(_lib.CONSTANTS['MCGEN_EVAL_WORK'], dtype=torch.float64, device=device)   # the first passes' partials
        self.count = 0

    def reset(self):
        self.state.zero_()
        self.count = 0

    def update(self, input, output):
        """One batch: launches only, nothing is synchronised.  n = input['img'].size(0), or the size of `output`'s first tensor
        that has a batch dimension (a loss has none) when `input` is None."""
        if input is not None:
            n = _tensor(input['img'], "input['img']").size(0)
        else:
            n = next(_tensor(v, 'output') for v in output.values() if torch.is_tensor(v) and v.dim() > 0).size(0)
        s = self.slot
        for name in self.names:
            if name in _SCALAR_KEY:
                value = _tensor(output[_SCALAR_KEY[name]], f"output['{_SCALAR_KEY[name]}']")
                ops.eval_scalar(value.float().reshape(1), n, self.acc, self.last, s[name])
        if any(name in s for name in _IMG):
            ops.eval_img(_tensor(output['img'], "output['img']"), _tensor(input['img'], "input['img']"), n, self.work, self.acc,
                         self.last, *(s.get(name, -1) for name in _IMG))
        if 'NLL' in s:
            ops.eval_nll(_tensor(output['logits'], "output['logits']"), _tensor(input['img'], "input['img']"), n, self.work,
                         self.acc, self.last, s['NLL'])
        if 'Accuracy' in s:
            ops.eval_accuracy(_tensor(output['label'], "output['label']"), _tensor(input['label'], "input['label']"), n,
                              self.work, self.acc, self.last, s['Accuracy'])
        self.count += n

    def repeat_last(self):
        """The last batch once more with n = 1: the reference's trailing `logger.append(evaluation, 'test')` (test_vae.py:72,
        test_glow.py:73, test_pixelcnn.py:80, test_vqvae.py:73)."""
        if self.count == 0:
            raise ValueError('Not valid state: repeat_last before the first update')
        self.acc.add_(self.last)
        self.count += 1

    def fetch(self):
        """(result(), last_values()) from one device-to-host copy."""
        if self.count == 0:
            raise ValueError('Not valid state: result before the first update')
        acc, last = self.state.tolist()
        return ({name: acc[i] / self.count for name, i in self.slot.items()}, {name: last[i] for name, i in self.slot.items()})

    def result(self):
        """{name: sum n_i v_i / sum n_i} as Python floats: one device-to-host copy."""
        return self.fetch()[0]

    def last_values(self):
        """{name: the last batch's value}: what `Logger.tracker` holds after the loop.  One device-to-host copy."""
        last = self.last.tolist()
        return {name: last[i] for name, i in self.slot.items()}
