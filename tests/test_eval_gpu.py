"""The device evaluation metrics (mcgen_amd.evaluate.DeviceEvaluator, csrc/eval_ops.hip) against their float64 restatement
(tests/eval_ref.py) and against the existing compat/metrics functions on the same device tensors.

Tolerances: 1e-9 relative against eval_ref, as in test_dbi_gpu.py -- the float32 inputs are read exactly and every sum is
float64 over at most 4e5 bounded terms, a forward error of about 1e-11, so 1e-9 leaves two orders for another summation order
and still catches any float32 accumulation (1e-7 at best); 1e-5 relative against compat/metrics, whose float32 formulas lie
within 1.2e-7 of the restatement on these shapes (test_eval_ref_cpu.py)."""
import functools
import math
import os
import struct
import sys

import pytest
import torch

import eval_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, 'compat') not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
RTOL64, RTOL32 = 1e-9, 1e-5


def _close(got, want, rtol, what=''):
    print(what, got, want, abs(got - want) / max(abs(want), 1e-300) if math.isfinite(want) else '')
    return got == want or abs(got - want) <= rtol * abs(want)


def _bits(values):
    return [struct.pack('<d', v) for v in values]


def _evaluate(names, input, output):
    from mcgen_amd.evaluate import DeviceEvaluator
    ev = DeviceEvaluator(names, 'cuda')
    ev.update(input, output)
    res, last = ev.result(), ev.last_values()                                      # one batch: its mean n * v / n is v, rounded twice
    assert all(r == v or abs(r - v) <= 4e-16 * abs(v) for r, v in zip(res.values(), last.values()) if v == v)
    return last


@functools.lru_cache(maxsize=None)
def _img_case(shape):
    out, tgt = R.image_pair(list(shape))
    return out, tgt, {'MSE': R.mse(out, tgt), 'BCE': R.bce(out, tgt), 'PSNR': R.psnr(out, tgt)}


@pytest.mark.parametrize('shape,offset', [(tuple(s), 0) for s in R.IMG_SHAPES] + [((5, 3, 7, 9), 1), ((11, 3, 31, 29), 1)], ids=str)
def test_image_metrics(shape, offset):
    """offset 1: both tensors are views one element into their storage, so the base address is only 4-byte aligned."""
    import metrics as M
    out, tgt, want = _img_case(shape)
    dev = []
    for t in (out, tgt):
        store = torch.empty(t.numel() + offset, device='cuda')
        store[offset:].copy_(t.view(-1))
        dev.append(store[offset:].view(t.shape))
        assert dev[-1].is_contiguous() and dev[-1].data_ptr() % 16 == 4 * offset
    input, output = {'img': dev[1]}, {'img': dev[0]}
    got = _evaluate(['MSE', 'BCE', 'PSNR'], input, output)
    for name in ('MSE', 'BCE', 'PSNR'):
        assert _close(got[name], want[name], RTOL64, name)
        single = _evaluate([name], input, output)[name]
        assert _bits([single]) == _bits([got[name]]), name                          # requested singly: the same bits
    assert _bits(_evaluate(['PSNR', 'MSE', 'BCE'], input, output)[n] for n in ('MSE', 'BCE', 'PSNR')) == \
        _bits(got[n] for n in ('MSE', 'BCE', 'PSNR'))                              # and again, in another slot order
    if want['MSE'] > 0:
        assert _close(got['MSE'], M.MSE(dev[0], dev[1]), RTOL32, 'compat MSE')
        assert _close(got['PSNR'], M.PSNR(dev[0], dev[1]), RTOL32, 'compat PSNR')
    assert _close(got['BCE'], M.BCE(dev[0], dev[1]), RTOL32, 'compat BCE')


@pytest.mark.parametrize('shape,scale', [(s, 1.0) for s in R.NLL_SHAPES] + [(R.NLL_SHAPES[0], 40.0)], ids=str)
def test_nll(shape, scale):
    """scale 40: logits of about +-150, where an exp without the maximum subtracted overflows float32."""
    import metrics as M
    logits, target = R.logit_map(shape, scale=scale)
    assert int(target.min()) == 0 and (target.numel() == 1 or int(target.max()) == shape[1] - 1)
    input, output = {'img': target.cuda()}, {'logits': logits.cuda()}
    got = _evaluate(['NLL'], input, output)['NLL']
    assert _close(got, R.nll(logits, target), RTOL64, 'NLL')
    assert _close(got, M.NLL(output['logits'], input['img']), RTOL32, 'compat NLL')
    assert _bits([_evaluate(['NLL'], input, output)['NLL']]) == _bits([got])


@pytest.mark.parametrize('shape', R.ACC_SHAPES, ids=str)
def test_accuracy(shape):
    import metrics as M
    logits, label = R.class_rows(shape)
    input, output = {'img': torch.zeros(shape[0], 1, device='cuda'), 'label': label.cuda()}, {'label': logits.cuda()}
    got = _evaluate(['Accuracy'], input, output)['Accuracy']
    assert _close(got, R.accuracy(logits, label), RTOL64, 'Accuracy')
    assert _close(got, M.Accuracy(output['label'], input['label']), RTOL32, 'compat Accuracy')


def test_accuracy_ties_and_nan():
    import metrics as M
    logits, label = R.class_rows((130, 100), seed=1)
    logits[0, 3] = logits[0, 7] = logits[1, 3] = logits[1, 7] = 9.0                # tied maxima: index 3 wins
    label[0], label[1] = 3, 7
    input, output = {'img': logits.cuda(), 'label': label.cuda()}, {'label': logits.cuda()}
    tied = _evaluate(['Accuracy'], input, output)['Accuracy']
    assert _close(tied, R.accuracy(logits, label), RTOL64, 'ties')
    two = _evaluate(['Accuracy'], {'img': logits[:2].cuda(), 'label': label[:2].cuda()}, {'label': logits[:2].cuda()})['Accuracy']
    assert two == 50.0                                                             # the first is a hit, the second a miss
    # a NaN in a row whose label is the row's maximum: a miss (torch.topk ranks the NaN first, so compat agrees here)
    logits[2, 11], logits[2, 50], label[2] = 20.0, float('nan'), 11
    output = {'label': logits.cuda()}
    input = dict(input, label=label.cuda())
    got = _evaluate(['Accuracy'], input, output)['Accuracy']
    assert _close(got, R.accuracy(logits, label), RTOL64, 'NaN row')
    assert _close(got, M.Accuracy(output['label'], input['label']), RTOL32, 'compat, NaN row')
    logits[2, 50] = 0.0
    assert R.accuracy(logits, label) > got                                         # without the NaN the row is a hit


def _sequence(ev, batches):
    for input, output in batches:
        ev.update(input, output)
    ev.repeat_last()
    return ev.result()


def test_accumulation_reset_and_independence():
    from mcgen_amd.evaluate import DeviceEvaluator
    names = ['Loss', 'MSE', 'BCE', 'PSNR']
    batches, want = [], R.Accumulator()
    for i, n in enumerate((5, 5, 3)):
        out, tgt = R.image_pair([n, 3, 7, 9], seed=10 + i)
        loss = torch.tensor(0.25 * (i + 1) + 1e-3)
        want.update({'Loss': float(loss), 'MSE': R.mse(out, tgt), 'BCE': R.bce(out, tgt), 'PSNR': R.psnr(out, tgt)}, n)
        batches.append(({'img': tgt.cuda()}, {'img': out.cuda(), 'loss': loss.cuda()}))
    want.repeat_last()
    ev, other = DeviceEvaluator(names, 'cuda'), DeviceEvaluator(['MSE'], 'cuda')
    other.update(*batches[1])                                                      # a second evaluator alive: no shared state
    got = _sequence(ev, batches)
    assert ev.count == want.count == 14
    for name in names:
        assert _close(got[name], want.result()[name], RTOL64, name)
        assert _close(ev.last_values()[name], want.last[name], RTOL64, 'last ' + name)
    assert ev.fetch() == (ev.result(), ev.last_values())                           # both from one copy
    assert _close(other.result()['MSE'], R.mse(batches[1][1]['img'], batches[1][0]['img']), RTOL64, 'other')
    ev.reset()
    assert ev.count == 0 and ev.acc.abs().sum().item() == 0 and ev.last.abs().sum().item() == 0
    again = _sequence(ev, batches)                                                 # the same sequence: identical bits
    assert _bits(again.values()) == _bits(got.values())
    assert other.count == 5


def test_nan_loss_propagates_and_input_none():
    from mcgen_amd.evaluate import DeviceEvaluator
    ev = DeviceEvaluator(['Loss', 'Loss_G', 'Loss_D'], 'cuda')
    ev.update(None, {'loss': torch.tensor(1.0).cuda(), 'loss_G': torch.tensor(2.0).cuda(), 'loss_D': torch.tensor(3.0).cuda(),
                     'img': torch.zeros(4, 1, 2, 2, device='cuda')})
    ev.update(None, {'loss': torch.tensor(float('nan')).cuda(), 'loss_G': torch.tensor(4.0).cuda(),
                     'loss_D': torch.tensor(-1.0).cuda(), 'img': torch.zeros(4, 1, 2, 2, device='cuda')})
    res = ev.result()
    assert ev.count == 8 and res['Loss'] != res['Loss'] and res['Loss_G'] == 3.0 and res['Loss_D'] == 1.0


def test_update_refuses_cpu_tensors_and_lists():
    from mcgen_amd.evaluate import DeviceEvaluator
    from mcgen_amd._lib import McgenError
    ev = DeviceEvaluator(['MSE'], 'cuda')
    x = torch.zeros(2, 1, 2, 2)
    with pytest.raises(ValueError, match='no CPU path'):
        ev.update({'img': x.cuda()}, {'img': x})
    with pytest.raises(ValueError, match='Not valid input type'):
        ev.update({'img': x.cuda()}, {'img': [x.cuda()]})
    with pytest.raises(McgenError, match='contiguous'):
        ev.update({'img': x.cuda()}, {'img': x.cuda().transpose(2, 3)})
    with pytest.raises(ValueError):
        ev.result()
