"""The float64 yardstick of the device evaluation metrics (tests/eval_ref.py) against the reference's own float32 formulas, and
the host-side parts of mcgen_amd.evaluate that need no GPU.

Tolerance 1e-5 relative: the float32 formulas (F.mse_loss, F.binary_cross_entropy on the mapped tensors, F.cross_entropy, the
topk accuracy of metrics.py:169-175) differ from the float64 restatement by at most 1.2e-7 relative on these shapes, so 1e-5
leaves two orders of margin."""
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

import eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, 'compat') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
RTOL32 = 1e-5


def _close(got, want, rtol):
    print(got, want, abs(got - want) / max(abs(want), 1e-300))
    return got == want or abs(got - want) <= rtol * abs(want)


@pytest.mark.parametrize('shape', R.IMG_SHAPES, ids=str)
def test_image_metrics_vs_float32_formulas(shape):
    out, tgt = R.image_pair(shape)
    assert _close(R.mse(out, tgt), float(F.mse_loss(out, tgt)), RTOL32)
    assert _close(R.bce(out, tgt), float(F.binary_cross_entropy((out + 1) / 2, (tgt + 1) / 2, reduction='mean')), RTOL32)
    assert _close(R.psnr(out, tgt), float(20 * torch.log10(torch.tensor(1.0) / torch.sqrt(F.mse_loss(out, tgt)))), RTOL32)


def test_bce_clamps_both_logs():
    out, tgt = R.image_pair([1, 1, 2, 2])                    # exactly the four corner pairs: 0, 100, 100, 0
    assert R.bce(out, tgt) == 50.0


@pytest.mark.parametrize('shape,scale', [(s, 1.0) for s in R.NLL_SHAPES] + [(R.NLL_SHAPES[0], 40.0)], ids=str)
def test_nll_vs_float32_formula(shape, scale):
    logits, target = R.logit_map(shape, scale=scale)
    assert int(target.min()) == 0 and (target.numel() == 1 or int(target.max()) == shape[1] - 1)
    assert _close(R.nll(logits, target), float(F.cross_entropy(logits, target, reduction='mean')), RTOL32)


@pytest.mark.parametrize('shape', R.ACC_SHAPES, ids=str)
def test_accuracy_vs_topk(shape):
    logits, label = R.class_rows(shape)
    hit = logits.topk(1, 1, True, True)[1].eq(label.view(-1, 1)).any(1)               # metrics.py:169-175
    assert _close(R.accuracy(logits, label), float(hit.float().mean() * 100.0), RTOL32)


def test_accuracy_ties_nan_and_bounds():
    logits = torch.zeros(3, 10)
    logits[:2, 3] = logits[:2, 7] = 2.0
    logits[2, 4] = float('nan')
    assert R.accuracy(logits[:2], torch.tensor([3, 7])) == 50.0                     # the first maximum only
    assert R.accuracy(logits, torch.tensor([3, 3, 4])) == pytest.approx(200.0 / 3)  # the NaN row is a miss
    assert R.accuracy(logits, torch.tensor([3, 10, 4])) != R.accuracy(logits, torch.tensor([3, 10, 4]))     # NaN
    assert R.nll(torch.zeros(1, 2, 1, 1), torch.tensor([[[2]]])) != R.nll(torch.zeros(1, 2, 1, 1), torch.tensor([[[2]]]))


def test_weighted_mean_and_repeat_last_equal_the_logger():
    """sum n_i v_i / sum n_i with the trailing n = 1 repeat is what compat/logger.Logger folds incrementally."""
    from logger import Logger
    g = torch.Generator().manual_seed(7)
    batches = [({'Loss': float(torch.randn((), generator=g)) * 3, 'BCE': float(torch.rand((), generator=g))}, n) for n in (5, 5, 3)]
    logger, ours = Logger('unused'), R.Accumulator()
    for values, n in batches:
        logger.append(values, 'test', n)
        ours.update(values, n)
    logger.append(batches[-1][0], 'test')
    ours.repeat_last()
    assert ours.count == logger.counter['test/Loss'] == 14
    for k, v in ours.result().items():
        assert abs(v - logger.mean['test/' + k]) <= 1e-15 * abs(logger.mean['test/' + k])


def test_evaluator_refuses_cpu_and_unknown_names():
    from mcgen_amd.evaluate import DeviceEvaluator, SUPPORTED
    for name in ('InceptionScore', 'FID', 'DBI'):
        with pytest.raises(ValueError, match='Loss, Loss_G, Loss_D, MSE, BCE, PSNR, NLL, Accuracy'):
            DeviceEvaluator(['Loss', name], 'cuda')
    with pytest.raises(ValueError, match='no CPU path'):
        DeviceEvaluator(['Loss'], 'cpu')
    assert SUPPORTED == ('Loss', 'Loss_G', 'Loss_D', 'MSE', 'BCE', 'PSNR', 'NLL', 'Accuracy')
    # update() looks at the tensors before anything is launched: an evaluator built without its device buffers shows it here
    ev = DeviceEvaluator.__new__(DeviceEvaluator)
    ev.names, ev.slot, ev.count = ['MSE'], {'MSE': 0}, 0
    x = torch.zeros(2, 1, 2, 2)
    with pytest.raises(ValueError, match='no CPU path'):
        ev.update({'img': x}, {'img': x})
    with pytest.raises(ValueError, match='no CPU path'):
        ev.update(None, {'img': x})


def test_wrappers_refuse_bad_tensors_before_the_launch():
    from mcgen_amd import ops
    from mcgen_amd._lib import McgenError
    x, s = torch.zeros(2, 3), torch.zeros(16, dtype=torch.float64)
    w = torch.zeros(512, dtype=torch.float64)
    with pytest.raises(ValueError, match='Not valid input'):
        ops.eval_img(x, torch.zeros(3, 2), 2, w, s, s, 0)
    with pytest.raises(ValueError, match='Not valid input'):
        ops.eval_nll(torch.zeros(2, 5, 3), torch.zeros(2, 4, dtype=torch.int64), 2, w, s, s, 0)
    with pytest.raises(ValueError, match='Not valid input'):
        ops.eval_accuracy(x, torch.zeros(3, dtype=torch.int64), 2, w, s, s, 0)
    with pytest.raises(ValueError, match='Not valid input'):
        ops.eval_scalar(x, 2, s, s, 0)
    with pytest.raises(ValueError, match='share'):
        ops.eval_img(x, x, 2, w, s, s, 0, 1, 0)                                      # MSE and PSNR into one slot
    with pytest.raises(McgenError, match='no CPU path'):
        ops.eval_img(x, x, 2, w, s, s, 0)
    with pytest.raises(McgenError, match='expected float32'):
        ops.eval_img(x.double(), x.double(), 2, w, s, s, 0)


def test_eval_symbols_are_declared_and_bound():
    from mcgen_amd import _lib
    names = ('mcgen_eval_img', 'mcgen_eval_nll', 'mcgen_eval_accuracy', 'mcgen_eval_scalar')
    with open(os.path.join(ROOT, 'include', 'mcgen_hip.h')) as f:
        text = f.read()
    assert sorted(set(re.findall(r'\bint\s+(mcgen_eval_\w+)\s*\(', text))) == sorted(names)
    for name in names:
        res, args = _lib.SYMBOLS[name]
        assert res is _lib.C.c_int and args[-1] is _lib.C.c_void_p                  # int return, trailing void* stream
    assert _lib.CONSTANTS['MCGEN_EVAL_WORK'] == 2 * _lib.CONSTANTS['MCGEN_EVAL_GROUPS']
    assert _lib.CONSTANTS['MCGEN_EVAL_SLOTS'] >= 8
    assert _lib.CONSTANTS['MCGEN_ABI_VERSION'] == 9 if 'MCGEN_ABI_VERSION' in _lib.CONSTANTS else True
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert all(hasattr(lib, name) for name in names) and lib.mcgen_abi_version() == 9
