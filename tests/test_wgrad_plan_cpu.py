"""The weight-gradient scheduler's host arithmetic (no GPU): the two split policies of mcgen_amd.ops against values pinned
from the commit before they became functions, and the slab-reduce record against hand-written mcgen_wreduce_t fields.

tests/golden/wgrad_plan.json holds inputs AND expected splits.  The expected values were produced once by the previous
commit's arithmetic (the body of ops._launch_multi from `def wq` to the end of the leftover loop, and the
`if splits is None:` block of ops.wgrad, copied verbatim into a throw-away script), never by ops._plan_multi /
ops._default_splits:
  real    -- the distinct layer sets of every mcgen_wgrad_multi launch of one bench.py run (capture + warm-up, batch 128,
             bf16) per workload, recorded on an MI355X through ops.MULTI_LOG plus each layer's paired flag; budget = its 256
             CUs.  13 sets (cifar10 2, coil100 2, mcglow 3, mcglow-cifar10 3, mcpixelcnn 3; mcvae queues no such launch).
             The copied arithmetic reproduced every recorded split before it was applied to the sweep.
  sweep   -- 240 synthetic sets (random.Random(20261017): 1-16 layers, m_tiles 1-4096, blocks 1-16, ksize 1 / 3, side
             8 / 16 / 32, paired or not; every sixth set shrunk to <= 4 layers of 1-12 tiles and 1-3 blocks so that the
             tile cap binds), each at budgets 256 and 64 = 480 cases.  Cases in which a situation occurs, counted in the
             generating run, per budget (256 / 64):
               the cap m_tiles // unit * unit limits a layer ......................... 34 / 34
               the all-minimum allocation already exceeds the budget ................. 1 / 137
               need() takes its `t <= fix` branch .................................... 0 / 0
             The last cannot occur through the planner: the bisection's bracket starts at lo = _WG_FIX, every time it
             probes (and the final hi) is > lo, and no layer's fixed part exceeds _WG_FIX -- the branch only guards the
             division.
  default -- the shapes of BIG_WG and of test_same_shape_layers_share_one_launch (tests/test_kernels_gpu.py), image-layer
             (c8) shapes at N = 128 / 1 / 256-paired, paired shapes, and fp32 shapes; CU count 256.
"""
import ctypes
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from mcgen_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'wgrad_plan.json')) as _f:
    PLAN = json.load(_f)


@pytest.mark.parametrize('group', ['real', 'sweep'])
def test_multi_planner_matches_the_pinned_splits(group):
    cases = PLAN[group]
    assert len(cases) >= (400 if group == 'sweep' else 13)
    if group == 'sweep':
        assert {c['budget'] for c in cases} == {256, 64}
    else:
        assert {c['workload'] for c in cases} == {'cifar10', 'coil100', 'mcglow', 'mcglow-cifar10', 'mcpixelcnn'}
    for c in cases:
        layers = [(m, b, ks, side, bool(paired)) for m, b, ks, side, paired in c['layers']]
        got = ops._plan_multi(layers, c['budget'])
        assert got == c['splits'], (c, got)
        assert all(type(s) is int for s in got)
        minimum = 0
        for (m_tiles, blocks, _, _, paired), sp in zip(layers, got):
            unit = 2 if paired else 1
            assert 1 <= sp <= max(unit, m_tiles // unit * unit), (c, got)
            assert sp % unit == 0, (c, got)
            minimum += unit * blocks
        if minimum <= c['budget']:
            assert sum(sp * l[1] for sp, l in zip(got, layers)) <= c['budget'], (c, got)


def test_default_split_count_matches_the_pinned_values():
    cases = PLAN['default']
    assert len(cases) >= 15 and any(c['c8'] for c in cases) and any(c['paired'] for c in cases) and any(not c['bf16'] for c in cases)
    for c in cases:
        n, h = c['n'], c['h']
        got = ops._default_splits((n * h * h + 127) // 128, c['cout'], (c['cin'] + 31) // 32, c['ksize'], c['bf16'], h, h, n,
                                  c['c8'], c['paired'], 256)
        assert type(got) is int and got == c['splits'], (c, got)


class _FakeTensor:
    """What ops._p / ops._f32 and a row slice read of a 2-d float32 device tensor: no device behind it."""
    is_cuda, dtype = True, torch.float32

    def __init__(self, ptr, rows=1, cols=1):
        self.ptr, self.rows, self.cols = ptr, rows, cols

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.ptr

    def __getitem__(self, s):
        start, stop, step = s.indices(self.rows)
        assert step == 1
        return _FakeTensor(self.ptr + 4 * self.cols * start, stop - start, self.cols)


def _fields(job):
    a = _lib.WReduce()
    ctypes.memset(ctypes.byref(a), 0xff, ctypes.sizeof(a))          # every field has to be written
    job.fill(a)
    return {name: getattr(a, name) for name, _ in _lib.WReduce._fields_}


def _layer(kind, cout, cin, cs, ks, grad, bias_grad, bias_grad2, second, alpha, accumulate, row_perm, row_scale, taps, c8, splits,
           slabs, bias_slabs):
    seg = SimpleNamespace(ksize=ks, x=SimpleNamespace(shape=(4, 8, 8, cs)))
    q = ops._PendingLayer(kind, None, seg, None, cout, cin, grad, bias_grad, bias_grad2, second, alpha, accumulate, row_perm, row_scale,
                          taps, c8, 2, 1, splits)
    q.slabs, q.bias_slabs = slabs, bias_slabs
    return q


def test_reduce_job_of_a_paired_layer_with_bias_gradient():
    """Two halves: each reduces its half of the slabs (6 of 12 splits; 4 bias-slab rows per split) into its own targets."""
    elems = 9 * 64 * 128
    slabs, bslabs = _FakeTensor(0x10000000, 12, elems), _FakeTensor(0x20000000, 48, 128)
    q = _layer('multi', 120, 60, 64, 3, _FakeTensor(0x1000), _FakeTensor(0x2000), _FakeTensor(0x3000),
               (_FakeTensor(0x4000), _FakeTensor(0x5000), None), 0.5, True, 1, _FakeTensor(0x6000), (0, 0), False, 12, slabs, bslabs)
    a, b = q.jobs()
    common = dict(splits=6, Cout=120, Cin=60, ksize=3, Cout_w=128, row_perm=1, accumulate=1, alpha=0.5, row_scale=0x6000, cin_slab=64,
                  tapcols=0, tap0=0, ntap_out=0)
    assert _fields(a) == dict(common, slabs=0x10000000, grad=0x1000, bias_slabs=0x20000000, bias_grad=0x2000, bias_grad2=0x3000)
    assert _fields(b) == dict(common, slabs=0x10000000 + 6 * elems * 4, grad=0x4000, bias_slabs=0x20000000 + 24 * 128 * 4,
                              bias_grad=0x5000, bias_grad2=None)
    # without bias slabs the bias targets are not passed, whatever the caller named
    q = _layer('multi', 120, 60, 64, 3, _FakeTensor(0x1000), None, _FakeTensor(0x3000), (_FakeTensor(0x4000), None, None), 0.5, True, 1,
               None, (0, 0), False, 12, slabs, None)
    for j, (sl, gr) in zip(q.jobs(), ((0x10000000, 0x1000), (0x10000000 + 6 * elems * 4, 0x4000))):
        assert _fields(j) == dict(common, row_scale=None, slabs=sl, grad=gr, bias_slabs=None, bias_grad=None, bias_grad2=None)


def test_reduce_job_of_a_tap_window_layer():
    """taps=(3, 3): the job carries the window; one job over all the splits; a c8 layer's job says so in `tapcols`."""
    slabs = _FakeTensor(0x10000000, 5, 9 * 32 * 16)
    q = _layer('batch', 16, 24, 32, 3, _FakeTensor(0x1000), None, None, None, 2.0, False, 0, None, (3, 3), False, 5, slabs, None)
    (j,) = q.jobs()
    want = dict(slabs=0x10000000, grad=0x1000, bias_slabs=None, bias_grad=None, bias_grad2=None, splits=5, Cout=16, Cin=24, ksize=3,
                Cout_w=16, row_perm=0, accumulate=0, alpha=2.0, row_scale=None, cin_slab=32, tapcols=0, tap0=3, ntap_out=3)
    assert _fields(j) == want
    q = _layer('single', 128, 3, 8, 3, _FakeTensor(0x1000), _FakeTensor(0x2000), None, None, 1.0, False, 1, None, (0, 0), True, 4,
               _FakeTensor(0x10000000, 4, 3 * 128 * 32), _FakeTensor(0x20000000, 16, 128))
    (j,) = q.jobs()
    assert _fields(j) == dict(want, bias_slabs=0x20000000, bias_grad=0x2000, splits=4, Cout=128, Cin=3, Cout_w=128, row_perm=1, alpha=1.0,
                              cin_slab=8, tapcols=1, tap0=0, ntap_out=0)


def test_retired_scheduler_switches_are_not_read():
    """MCGEN_SIDE_STREAM, MCGEN_WG_W16 / _W8, MCGEN_WGRAD_TARGET_SMALL and MCGEN_WGRAD_BIG_TILES selected nothing and are gone:
    even under MCGEN_TUNING=1 nothing reads them."""
    code = ('import sys; sys.path.insert(0, %r)\n'
            'from mcgen_amd import ops, _tuning\n'
            'print(sorted(_tuning.ACTIVE.items()))\n') % ROOT
    env = {k: v for k, v in os.environ.items() if not k.startswith('MCGEN_')}
    env.update(MCGEN_TUNING='1', MCGEN_SIDE_STREAM='1', MCGEN_WG_W8='2', MCGEN_WG_W16='2', MCGEN_WGRAD_TARGET_SMALL='64',
               MCGEN_WGRAD_BIG_TILES='8')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split('\n')[-2] == '[]', r.stdout
