"""The weight-gradient kernels against the exact float64 reference of tests/conv_exact_ref.py (wgrad_ref).

On dyadic inputs (x and dy multiples of 1/4, scales 0.5 / 1 / 2, codes 0 / 0.5 / 1 / 2) every product and every partial
sum over pixels is an fp32 number (`assert_exact` on the reference's bit count), so after mcgen_wgrad_reduce(_batch) the
gradient must EQUAL alpha * sum dy * prologue(x) -- in fp32 and in bf16 alike (the slabs are fp32 either way), whatever
the split count and the reduce order.  One smallest case per kernel family:

  general mcgen_wgrad   few-tile form (fewer than 4 tiles per split), fp32 and bf16; the producer / consumer forms
                        (>= 4 tiles per split): bf16 ring (tiles inside one image), the fp32 / small-map pc kernel, the
                        1x1 chunk groups (>= 4 chunks)
  wgrad_c8              the image layers, 3x3 and 1x1 (with dy_ups), compact slabs reduced with tapcols
  mcgen_wgrad_multi     N = 2 on 8x8 maps, Cout 128, Cin 64; with a 16x16 layer in the same launch; with halves
  mcgen_wgrad_batch     two equal layers
Options: x ups, dy_ups, the prologue triple with non-binary codes, alpha != 1, accumulate onto a dyadic gradient, bias
slabs into bias_grad and bias_grad2.
"""
import pytest
import torch

import conv_exact_ref as R

pytestmark = pytest.mark.gpu


def _w(name, n, h, cin, cout, ksize, **kw):
    return dict(name=name, N=n, H=h, Cin=cin, Cout=cout, ksize=ksize, **kw)


# 128-pixel tiles: `tiles` = N H W / 128; the few-tile form runs below 4 tiles per split
CASES = [
    _w('few tiles f32', 3, 8, 16, 24, 3, dtype='f32', splits=2),                                     # 1.5 tiles: ragged
    _w('few tiles bf16 prologue', 3, 8, 16, 24, 3, splits=2, prologue=1, alpha=0.5, accumulate=1, bias=2),
    _w('few tiles bf16 1x1 ups', 4, 8, 40, 24, 1, splits=1, ups=1, bias=1),
    _w('few tiles f32 dy_ups', 2, 16, 8, 40, 3, dtype='f32', splits=2, dy_ups=1, prologue=1, bias=1),
    _w('ring bf16', 8, 16, 40, 72, 3, splits=2, prologue=1, alpha=0.25, accumulate=1, bias=2),       # 16 tiles, 8 per split
    _w('ring bf16 ups', 8, 16, 64, 40, 3, splits=2, ups=1, bias=1),
    _w('ring bf16 dy_ups', 8, 16, 32, 72, 3, splits=4, dy_ups=1, prologue=1),
    _w('ring bf16 1x1 dy_ups', 8, 16, 96, 40, 1, splits=2, dy_ups=1, accumulate=1, bias=1),
    _w('pc f32', 8, 16, 40, 72, 3, dtype='f32', splits=2, prologue=1, alpha=0.5, bias=2),
    _w('pc bf16 4x4 maps', 32, 4, 24, 40, 3, splits=1, prologue=1, accumulate=1),                     # tiles of 8 images: no ring
    _w('pc bf16 1x1 chunk groups', 8, 8, 160, 40, 1, splits=1, prologue=1, bias=1),                  # 5 chunks: a group of 4 + 1
    _w('ring bf16 8x16 maps', 16, 8, 40, 24, 3, W=16, splits=2, prologue=1, bias=1),                # non-square: 128-pixel tiles = whole images
    _w('few tiles bf16 1x1 maps', 16, 1, 128, 64, 1, splits=1, prologue=1, bias=1),                  # a Linear layer: one pixel per image
    _w('pc f32 2x2 maps', 160, 2, 16, 24, 1, dtype='f32', splits=1, accumulate=1),                   # 5 tiles of 32 images
    _w('c8 3x3', 2, 32, 8, 128, 3, splits=4, alpha=0.5, accumulate=1, bias=2, family='c8'),
    _w('c8 1x1 dy_ups', 2, 32, 8, 128, 1, splits=4, dy_ups=1, bias=1, family='c8'),
]
SPLIT_CASE = _w('splits', 8, 16, 40, 72, 3, prologue=1, bias=1)                                       # run at 2, 4 (ring) and 8 (few-tile)
MULTI_CASES = [
    _w('multi 8x8', 2, 8, 64, 128, 3, prologue=1, alpha=0.5, accumulate=1, bias=2),
    _w('multi 16x16', 2, 16, 64, 128, 3, ups=1, bias=1),
    _w('multi 8x8 dy_ups', 2, 8, 128, 128, 3, dy_ups=1),
    _w('multi halves', 4, 8, 64, 128, 3, prologue=1, bias=1, halves=1),
]
BATCH_CASES = [_w('batch a', 4, 8, 40, 24, 3, prologue=1, bias=1), _w('batch b', 4, 8, 40, 24, 3, prologue=1, bias=1, accumulate=1)]
ALL_CASES = CASES + [SPLIT_CASE] + MULTI_CASES + BATCH_CASES


def _ops():
    from mcgen_amd import ops
    return ops


class _Layer:
    """One layer's device operands and its exact expectation."""

    def __init__(self, ops, case, seed):
        c = self.case = case
        self.dtype = torch.float32 if c.get('dtype') == 'f32' else torch.bfloat16
        gen = torch.Generator(device='cuda').manual_seed(seed)
        ks, pro = c['ksize'], c.get('prologue', 0)
        t = R.wgrad_inputs(gen, c['N'], c['H'], c.get('W', c['H']), c['Cin'], c['Cout'], ks, ups=c.get('ups', 0), dy_ups=c.get('dy_ups', 0), prologue_on=pro)
        self.alpha, self.acc, self.bias = c.get('alpha', 1.0), c.get('accumulate', 0), c.get('bias', 0)
        if c.get('halves'):
            h = c['N'] // 2
            lo, hi = ({k: (v[:h] if k in ('x', 'dy', 'code') else v) for k, v in t.items()},
                      {k: (v[h:] if k in ('x', 'dy', 'code') else v) for k, v in t.items()})
            self.want = [R.wgrad_ref(q, ks, c.get('ups', 0), c.get('dy_ups', 0), pro, self.alpha) for q in (lo, hi)]
        else:
            self.want = [R.wgrad_ref(t, ks, c.get('ups', 0), c.get('dy_ups', 0), pro, self.alpha)]
        for _, _, bits in self.want:
            R.assert_exact(bits, c['name'])
        f = lambda k: t[k].float().contiguous() if k in t else None
        self.seg = ops.Seg(t['x'].to(self.dtype).contiguous(), ksize=ks, scale=f('scale'), shift=f('shift'), code=f('code'),
                           ups=bool(c.get('ups', 0)), relu=bool(pro))
        self.dy = t['dy'].to(self.dtype).contiguous()
        self.g0, self.b0 = t['grad0'], t['bias0']
        init = lambda v: v.float().clone() if self.acc else torch.full_like(v, 7.0).float()       # (overwritten without accumulate)
        n_out = 2 if c.get('halves') else 1
        self.grads = [init(self.g0) for _ in range(n_out)]
        self.bgs = [[init(self.b0) for _ in range(self.bias)] for _ in range(n_out)]

    def launch(self, ops, splits=None):
        c = self.case
        bg = lambda i, j: self.bgs[i][j] if self.bias > j else None
        second = (self.grads[1], bg(1, 0), bg(1, 1)) if c.get('halves') else None
        ops.wgrad(self.seg, self.dy, c['Cout'], c['Cin'], self.grads[0], dy_ups=bool(c.get('dy_ups', 0)), alpha=self.alpha,
                  accumulate=bool(self.acc), splits=splits, bias_grad=bg(0, 0), bias_grad2=bg(0, 1), second=second)

    def check(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:               # a device-side fault: nothing more is launched on a faulted GPU
            pytest.exit(f'GPU fault, stopping the session: {e}', returncode=3)
        for i, (dw, db, _) in enumerate(self.want):
            wg = ((self.g0 if self.acc else 0) + dw).float()
            wb = ((self.b0 if self.acc else 0) + db).float()
            g = self.grads[i]
            assert torch.equal(g, wg), f"{self.case['name']}: {int((g != wg).sum())} of {g.numel()} weight-gradient entries differ, " \
                                       f"max |diff| {float((g - wg).abs().max()):.3e}"
            for b in self.bgs[i]:
                assert torch.equal(b, wb), f"{self.case['name']}: bias gradient differs by {float((b - wb).abs().max()):.3e}"


@pytest.mark.parametrize('case', CASES, ids=lambda c: c['name'])
def test_wgrad_exact(case):
    ops = _ops()
    layer = _Layer(ops, case, 11 + len(case['name']))
    ops.WGRAD_LOG = log = []
    try:
        layer.launch(ops, case['splits'])
    finally:
        ops.WGRAD_LOG = None
    assert log == [case.get('family', 'general')]
    layer.check()


def test_split_count_and_reduce_order_do_not_matter():
    ops = _ops()
    out = []
    for splits in (2, 4, 8, 16):                  # 16 tiles: 8 / 4 per split (ring form), 2 / 1 per split (few-tile form)
        layer = _Layer(ops, SPLIT_CASE, 99)
        layer.launch(ops, splits)
        layer.check()
        out.append((layer.grads[0], layer.bgs[0][0]))
    for g, b in out[1:]:
        assert torch.equal(g, out[0][0]) and torch.equal(b, out[0][1])


@pytest.mark.parametrize('names', [('multi 8x8',), ('multi 8x8', 'multi 16x16', 'multi 8x8 dy_ups'), ('multi halves', 'multi 8x8')],
                         ids=['one layer', 'with a 16x16 layer', 'halves'])
def test_wgrad_multi_exact(names):
    ops = _ops()
    layers = [_Layer(ops, c, 31 + i) for i, c in enumerate(MULTI_CASES) if c['name'] in names]
    ops.MULTI_LOG = log = []
    try:
        with ops.deferred_reduces():
            for layer in layers:
                layer.launch(ops)
    finally:
        ops.MULTI_LOG = None
    assert len(log) == 1 and len(log[0]) == len(layers), log          # ONE mcgen_wgrad_multi launch with every layer
    for layer in layers:
        layer.check()


def test_wgrad_batch_exact():
    ops = _ops()
    layers = [_Layer(ops, c, 51 + i) for i, c in enumerate(BATCH_CASES)]
    ops.BATCH_LOG = log = []
    try:
        with ops.deferred_reduces():
            for layer in layers:
                layer.launch(ops)
    finally:
        ops.BATCH_LOG = None
    assert log == [2], log                                            # one mcgen_wgrad_batch launch of two layers
    for layer in layers:
        layer.check()
