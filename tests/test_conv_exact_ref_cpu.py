"""The exact-arithmetic sweep's reference, inputs and case tables, checked without a GPU (tests/conv_exact_ref.py):

  * conv_ref / wgrad_ref against F.conv2d, F.avg_pool2d and autograd in float64 on Gaussian (non-dyadic) data: the
    reference checked as mathematics, every option singly and the two ordering combinations;
  * the exactness condition (every partial sum within fp32's 24 bits) for every (case, option) pair of the GPU tables,
    and that it trips on a deliberately over-deep case;
  * coverage, through mcgen_conv_plan (no HIP call): the base cases reach every row of the fp32 and the shipped bf16
    table and every variant of the kernels in files of their own -- INSTANTIATIONS pins, per case, what it reaches, so a
    row no case reaches (or a deleted case) fails by being absent;
  * tests/golden/conv_exact_routes.json pins the plan's answer for every (case, option) pair: keeps the route, falls to
    another, or refuses.  A change to a *_ok line moves this file.  `python tests/test_conv_exact_ref_cpu.py --write`
    rewrites it from the current library.
"""
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                     # (run as a script to rewrite the fixture: pytest's conftest does this otherwise)
    sys.path.insert(0, ROOT)

import conv_exact_ref as R  # noqa: E402

ROUTES_JSON = os.path.join(ROOT, 'tests', 'golden', 'conv_exact_routes.json')


# ---- the reference against torch ----------------------------------------------------------------------------------------
def _nchw(x):
    return x.permute(0, 3, 1, 2)


def torch_conv(c, t):
    """The header's contract restated with torch.nn.functional on NCHW tensors; returns (v, sum0, sum1) in NHWC / [Cout]."""
    n = c['N']
    acc = 0
    for i, s in enumerate(c['segs']):
        a = _nchw(t[f'x{i}'])
        if s['ups']:
            a = F.interpolate(a, scale_factor=2, mode='nearest')
        if s['affine']:
            sc, sh = t[f'scale{i}'], t[f'shift{i}']
            if s['group_n']:
                sc, sh = sc.repeat_interleave(s['group_n'], 0), sh.repeat_interleave(s['group_n'], 0)
                a = a * sc[:, :, None, None] + sh[:, :, None, None]
            else:
                a = a * sc[None, :, None, None] + sh[None, :, None, None]
        if s['relu']:
            a = F.relu(a)
        if s['code']:
            a = a * t[f'code{i}'][:, :, None, None]
        w = t[f'w{i}']
        if w.dim() == 5:
            acc = acc + torch.cat([F.conv2d(a[j:j + 1], w[int(t['wsel'][j])], padding=s['ksize'] // 2) for j in range(n)])
        else:
            acc = acc + F.conv2d(a, w, padding=s['ksize'] // 2)
    if c['pool']:
        acc = F.avg_pool2d(acc, 2) * 4
    v = c['alpha'] * acc
    for k in ('bias', 'bias2'):
        if c[k]:
            v = v + t[k][None, :, None, None]
    if c['ocode']:
        v = v * t['ocode'][:, :, None, None]
    s0 = s1 = None
    if c['gate']:
        gx = _nchw(t['gate_x'])
        z = (gx * t['gscale'][None, :, None, None] + t['gshift'][None, :, None, None]) if c['gate'] == 2 else gx
        # the gate IS the derivative of the forward ReLU: take it from autograd
        z = z.clone().requires_grad_(True)
        (F.relu(z) * v).sum().backward()
        v = z.grad
    if c['stats_mode'] == 2:
        xhat = (_nchw(t['gate_x']) - t['gmean'][None, :, None, None]) * t['grstd'][None, :, None, None]
        s0, s1 = v.sum((0, 2, 3)), (v * xhat).sum((0, 2, 3))
    if c['res']:
        v = v + _nchw(t['res'])
    if c['tanh_out']:
        v = torch.tanh(v)
    if c['stats_mode'] == 1:
        s0, s1 = v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))
    return v.permute(0, 2, 3, 1), s0, s1


SMALL = [
    dict(name='3x3', N=4, H=8, W=8, Cout=12, segs=[dict(C=8)]),
    dict(name='1x1 8x16', N=2, H=8, W=16, Cout=5, segs=[dict(C=16, ksize=1)]),
    dict(name='two segments', N=4, H=4, W=4, Cout=8, segs=[dict(C=8, affine=1, relu=1, code=1), dict(C=16, ksize=1, ups=1, code=1)]),
    dict(name='weight sets', N=5, H=4, W=4, Cout=8, segs=[dict(C=8)], wsel=3),
]


@pytest.mark.parametrize('option', R.SWEEP)
@pytest.mark.parametrize('base', SMALL, ids=lambda b: b['name'])
def test_conv_ref_is_the_headers_contract(base, option):
    c = R.apply_option(base, option)
    if c is None:                                # (the option does not apply to this shape: nothing to compare)
        return
    gen = torch.Generator().manual_seed(len(option) * 131 + len(base['name']))
    t = R.real_inputs(gen, c)
    r = R.conv_ref(c, t)
    v, s0, s1 = torch_conv(c, t)
    torch.testing.assert_close(r['v'], v, rtol=1e-12, atol=1e-12)
    assert bool((r['S'] + 1e-12 >= r['pre'].abs()).all())
    if c['stats_mode']:
        torch.testing.assert_close(r['sums'][0], s0, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(r['sums'][1], s1, rtol=1e-12, atol=1e-12)
    else:
        assert r['sums'] is None


def test_the_two_orders_are_told_apart():
    """On the dyadic inputs a swapped epilogue order changes the exact result: the sums with and without `res`, with and
    without the output code / the tanh differ, so a kernel that takes them at the wrong place cannot pass."""
    base = dict(name='o', N=4, H=8, W=8, Cout=16, segs=[dict(C=8)])
    gen = torch.Generator().manual_seed(5)
    c = R.apply_option(base, 'order_bwd')
    t = R.exact_inputs(gen, c)
    r = R.conv_ref(c, t)
    with_res = r['v'].sum((0, 1, 2))
    assert not torch.equal(r['sums'][0], with_res)                           # sums in front of `res`
    no_code = R.conv_ref(dict(c, ocode=0), t)['sums'][0]
    assert not torch.equal(r['sums'][0], no_code)                            # ... behind the code
    no_gate = R.conv_ref(dict(c, gate=0, stats_mode=1, res=0), t)['sums'][0]
    assert not torch.equal(r['sums'][0], no_gate)                            # ... and behind the gate
    # (a code that is not 0 / 1: a kernel that treats it as a flag fails)
    assert set(t['ocode'].unique().tolist()) == {0.0, 0.5, 1.0, 2.0}
    c = R.apply_option(base, 'order_fwd')
    t = R.exact_inputs(gen, c)
    r = R.conv_ref(c, t)
    assert not torch.equal(r['sums'][0], r['pre'].sum((0, 1, 2)))            # the forward sums see the tanh
    assert not torch.equal(r['pre'], R.conv_ref(dict(c, res=0), t)['pre'])


@pytest.mark.parametrize('ks,ups,dy_ups,pro', [(3, 0, 0, 0), (3, 1, 0, 1), (3, 0, 1, 1), (1, 0, 0, 1), (1, 1, 1, 0)])
def test_wgrad_ref_is_autograd(ks, ups, dy_ups, pro):
    gen = torch.Generator().manual_seed(7 + ks + ups)
    n, h, w, ci, co = 3, 8, 8, 8, 12
    t = R.wgrad_inputs(gen, n, h, w, ci, co, ks, ups=ups, dy_ups=dy_ups, prologue_on=pro)
    for k in ('x', 'dy') + (('scale', 'shift', 'code') if pro else ()):
        t[k] = torch.randn(t[k].shape, generator=gen, dtype=torch.float64)
    dw, db, _ = R.wgrad_ref(t, ks, ups=ups, dy_ups=dy_ups, relu=pro, alpha=0.5)
    a = _nchw(t['x'])
    if ups:
        a = F.interpolate(a, scale_factor=2, mode='nearest')
    if pro:
        a = F.relu(a * t['scale'][None, :, None, None] + t['shift'][None, :, None, None]) * t['code'][:, :, None, None]
    dy = _nchw(t['dy'])
    if dy_ups:
        dy = F.interpolate(dy, scale_factor=2, mode='nearest')
    wt = torch.zeros(co, ci, ks, ks, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(co, dtype=torch.float64, requires_grad=True)
    (F.conv2d(a, wt, b, padding=ks // 2) * dy).sum().backward()
    torch.testing.assert_close(dw, 0.5 * wt.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db, 0.5 * b.grad, rtol=1e-12, atol=1e-12)


# ---- the exactness condition -------------------------------------------------------------------------------------------
PAIRS = R.pairs()


def _cost(c):
    return c['N'] * c['H'] * c['W'] * c['Cout'] * sum(s['ksize'] ** 2 * (s['Cw'] or s['C']) for s in c['segs'])


def test_every_case_of_the_tables_is_exact():
    """bound_bits (|a|, |w| by their maxima: no convolution) for every pair; the full reference -- accumulation, epilogue
    and the per-tile column sums -- where a CPU can afford it.  The GPU test asserts the full condition for every pair."""
    checked = 0
    for name, opt, c in PAIRS:
        if c is None:
            continue
        gen = torch.Generator().manual_seed(checked)
        if _cost(c) <= 2e7:
            t = R.exact_inputs(gen, c)
            r = R.conv_ref(c, t)
            R.assert_exact(r['bits'], f'{name} / {opt}')
            assert R.bound_bits(c, t) >= R._bits(float(r['S'].max()), r['q']) - 1
        else:
            small = R.full(dict(c, N=max(c['y_group'], 2)))                            # the bound does not depend on N
            if small['segs'][0]['group_n']:
                small['segs'][0]['group_n'] = small['N']
            t = R.exact_inputs(gen, small)
            c = small
        R.assert_exact(R.bound_bits(c, t), f'{name} / {opt}')
        for i, s in enumerate(c['segs']):                                             # 8 significant bits: exact in bf16
            a = R.prologue(t[f'x{i}'], t.get(f'scale{i}'), t.get(f'shift{i}'), s['relu'], t.get(f'code{i}'), s['ups'], s['group_n'])
            assert torch.equal(a.bfloat16().double(), a), (name, opt)
        checked += 1
    assert checked > 1400


def test_wgrad_cases_are_exact():
    import test_wgrad_exact_gpu as W
    for case in W.ALL_CASES:
        gen = torch.Generator().manual_seed(1)
        t = R.wgrad_inputs(gen, case['N'], case['H'], case.get('W', case['H']), case['Cin'], case['Cout'], case['ksize'], ups=case.get('ups', 0),
                           dy_ups=case.get('dy_ups', 0), prologue_on=case.get('prologue', 0), xr=case.get('xr', 4))
        _, _, bits = R.wgrad_ref(t, case['ksize'], ups=case.get('ups', 0), dy_ups=case.get('dy_ups', 0), relu=case.get('prologue', 0),
                                 alpha=case.get('alpha', 1.0))
        R.assert_exact(bits, case['name'])


def test_an_over_deep_case_is_not_exact():
    c = R.full(dict(name='deep', N=1, H=4, W=4, Cout=8, xr=128, segs=[dict(C=4096, affine=1, code=1)]))
    t = R.exact_inputs(torch.Generator().manual_seed(3), c)
    r = R.conv_ref(c, t)
    assert r['bits'] > 24 and R.bound_bits(c, t) >= r['bits']
    with pytest.raises(AssertionError):
        R.assert_exact(r['bits'], 'deep')


# ---- coverage -----------------------------------------------------------------------------------------------------------
def instantiation(c):
    """Which kernel instantiation a case reaches: the plan's answer, plus -- for what the plan does not report -- the
    template parameter or launch form the case's shape selects inside that route."""
    a = R.answer(c)
    route = a.split('/')[0]
    if a.startswith('refused'):
        return a
    if route == 'skinny':
        a += f"/W{c['W']}"
    elif route == 'smap':
        sig = '+'.join(f"{s['C']}k{s['ksize']}" + ('u' if s['ups'] else '') for s in c['segs'])
        a += f"/{sig}/" + ('pair' if c['N'] % 2 == 0 and c['N'] * (c['Cout'] // 64) >= 512 else 'single')
    elif route == 'px1':
        a += f"/{c['H']}x{c['W']}"
    elif route == 'c8':
        a += '/whole' if c['N'] >= 192 else '/half'
    elif a.endswith('/20') or route == 'gk-pp':
        a += f"/W{c['W']}"                                  # (the pp kernel is instantiated per map width)
    for flag in ('wsel', 'order', 'ycmap', 'yperm', 'y_group'):
        if c[flag]:
            a += '+' + flag
    return a


INSTANTIATIONS = {         # case of conv_exact_ref.BASE_CASES / MODE_CASES -> what it reaches
    'f32 128x16': 'tiled/128x16/0',
    'f32 64x64': 'tiled/64x64/0',
    'f32 64x64 8x16': 'tiled/64x64/0',
    'f32 128x128': 'tiled/128x128/0',
    '64x64': 'tiled/64x64/11',
    '64x64 8x16': 'tiled/64x64/11',
    '64x64 4x4': 'tiled/64x64/11',
    '64x64 1x1 map': 'tiled/64x64/11',
    '64x16 cp': 'tiled/64x16/12',
    '64x16 cp 4x4': 'tiled/64x16/12',
    '128x16 cp': 'tiled/128x16/12',
    '256x16': 'tiled/256x16/5',
    '64x128': 'tiled/64x128/5',
    '64x64 grouped 1x1': 'tiled/64x64/11/g',
    '128x64': 'tiled/128x64/5',
    '128x64 whole': 'tiled/128x64/5',
    '128x128': 'tiled/128x128/5',
    '128x128 whole': 'tiled/128x128/5',
    '256x128 pp': 'tiled/256x128/20/W32',
    '256x128 pp whole': 'tiled/256x128/20/W32',
    '256x128 pp W16': 'tiled/256x128/20/W16',
    '128x256': 'tiled/128x256/5',
    '128x256 pp': 'tiled/128x256/20/W32',
    '128x256 pp W16': 'tiled/128x256/20/W16',
    '256x256': 'tiled/256x256/5',
    '256x256 pp': 'tiled/256x256/20/W32',
    '256x256 pp W16': 'tiled/256x256/20/W16',
    '64x16 cp W32': 'tiled/64x16/12',
    '64x16 cp deep 1x1': 'tiled/64x16/12',
    '128x128 grouped 1x1': 'tiled/128x128/5/g',
    'map 16x2': 'tiled/64x64/11',
    'map 2x32': 'tiled/64x64/11',
    'map 1x16': 'tiled/64x64/11',
    'map 2x64': 'tiled/128x16/12',
    'f32 map 2x32': 'tiled/64x64/0',
    'f32 map 2x64': 'tiled/128x16/0',
    '128x64 8x8 ragged': 'tiled/128x64/5',
    '128x128 8x8 ragged': 'tiled/128x128/5',
    '256x256 8x8 ragged': 'tiled/256x256/5',
    '256x16 8x8 ragged': 'tiled/256x16/5',
    '128x128 W64': 'tiled/128x128/5',
    'f32 128x128 W64': 'tiled/128x128/0',
    '256x256 pp 16x32': 'tiled/256x256/20/W32',
    'skinny W4': 'skinny/W4',
    'skinny W8': 'skinny/W8',
    'skinny W16': 'skinny/W16',
    'smap 128k3': 'smap/128k3/single',
    'smap 128k3 pair': 'smap/128k3/pair',
    'smap 256k3': 'smap/256k3/single',
    'smap 256k3 pair': 'smap/256k3/pair',
    'smap 128k1': 'smap/128k1/single',
    'smap 128k1 pair': 'smap/128k1/pair',
    'smap 256k1': 'smap/256k1/single',
    'smap 256k1 pair': 'smap/256k1/pair',
    'smap 256k1+128k3': 'smap/256k1+128k3/single',
    'smap 256k1+128k3 pair': 'smap/256k1+128k3/pair',
    'smap 256k3+256k1ups': 'smap/256k3+256k1u/single',
    'smap 256k3+256k1ups pair': 'smap/256k3+256k1u/pair',
    'px1 16x16': 'px1/16x16',
    'px1 8x8': 'px1/8x8',
    'px1 4x4': 'px1/4x4',
    'c8 half images': 'c8/half',
    'c8 whole images': 'c8/whole',
    'head': 'head',
    'mc 128x128': 'mc/128x128/0',
    'mc 128x256': 'mc/128x256/0',
    'mc 256x256': 'mc/256x256/0',
    'gk dense 128x128': 'gk/128x128/0',
    'gk dense W64': 'gk/128x128/0',
    'gk 128x128': 'gk/128x128/0',
    'gk 128x256': 'gk/128x256/0',
    'mc 256x256 whole': 'mc/256x256/0',
    'gk 256x256': 'gk/256x256/0',
    'gk-pp': 'gk-pp/256x256/0/W32',
    'gk-pp whole': 'gk-pp/256x256/0/W32',
    'gk-pp W16': 'gk-pp/256x256/0/W16',
    'wsel': 'tiled/256x256/20/W32+wsel',
    'wsel whole': 'tiled/256x256/20/W32+wsel',
    'wsel + order': 'tiled/256x256/20/W32+wsel+order',
    'ycmap 256x256': 'tiled/256x256/5+ycmap',
    'ycmap pp': 'tiled/256x256/20/W32+ycmap',
    'ycmap 64x64': 'tiled/64x64/11+ycmap',
    'yperm 256x256': 'tiled/256x256/20/W32+wsel+yperm',
    'yperm 256x128': 'tiled/256x128/20/W32+wsel+yperm',
    'head wsel': 'head+wsel',
    'head y_group': 'head+y_group',
    'head wsel y_group': 'head+wsel+y_group',
}


def test_base_cases_reach_every_instantiation():
    got = {}
    for b in R.BASE_CASES + R.MODE_CASES:
        got[b['name']] = instantiation(R.full({k: v for k, v in b.items() if k != 'options'}))
    assert got == INSTANTIATIONS
    reached = set(got.values())
    # every shipped row / variant, written out once: a row no case reaches fails here by being absent
    rows_f32 = {'tiled/128x16/0', 'tiled/64x64/0', 'tiled/128x128/0'}
    rows_bf16 = {'tiled/256x256/5', 'tiled/128x256/5', 'tiled/128x128/5', 'tiled/64x128/5', 'tiled/64x64/11', 'tiled/256x16/5',
                 'tiled/64x16/12', 'tiled/128x16/12', 'tiled/256x256/20/W32', 'tiled/256x256/20/W16', 'tiled/256x128/20/W32',
                 'tiled/256x128/20/W16', 'tiled/128x256/20/W32', 'tiled/128x256/20/W16', 'tiled/128x64/5', 'tiled/64x64/11/g'}
    kmajor = {f'{r}/{t}/0' for r in ('mc', 'gk') for t in ('256x256', '128x256', '128x128')} | {'gk-pp/256x256/0/W32', 'gk-pp/256x256/0/W16'}
    sides = {'skinny/W4', 'skinny/W8', 'skinny/W16', 'px1/16x16', 'px1/8x8', 'px1/4x4', 'c8/half', 'c8/whole',
             'head', 'head+wsel', 'head+y_group', 'head+wsel+y_group'}
    sides |= {f'smap/{sig}/{k}' for sig in ('128k3', '256k3', '128k1', '256k1', '256k1+128k3', '256k3+256k1u') for k in ('pair', 'single')}
    modes = {'tiled/256x256/20/W32+wsel', 'tiled/256x256/20/W32+wsel+order', 'tiled/256x256/5+ycmap', 'tiled/256x256/20/W32+ycmap',
             'tiled/64x64/11+ycmap', 'tiled/256x256/20/W32+wsel+yperm', 'tiled/256x128/20/W32+wsel+yperm'}
    missing = (rows_f32 | rows_bf16 | kmajor | sides | modes) - reached
    assert not missing, missing
    # ... and the rows come from the plan: the dtype of the case decides which table a row belongs to
    f32 = {instantiation(R.full(b)) for b in R.BASE_CASES if b.get('dtype') == 'f32'}
    assert f32 == rows_f32


# ---- the plan's answer for every (case, option) pair --------------------------------------------------------------------
def route_triples():
    return [[name, opt, 'n/a' if c is None else R.answer(c)] for name, opt, c in PAIRS]


def test_route_answers_are_pinned():
    with open(ROUTES_JSON) as f:
        pinned = json.load(f)['answers']
    got = route_triples()
    assert len(got) == len(pinned), (len(got), len(pinned))
    moved = [(g, p) for g, p in zip(got, pinned) if g != p]
    assert not moved, moved[:10]
    # the three kinds of answer all occur: keeps the route, falls to another one, refuses
    base = {name: a.split('/')[0] for name, opt, a in got if opt == 'base'}
    kinds = {('refused' if a.startswith('refused') else 'keeps' if a.split('/')[0] == base[name] else 'falls') for name, opt, a in got if a != 'n/a'}
    assert kinds == {'keeps', 'falls', 'refused'}


if __name__ == '__main__' and '--write' in sys.argv:
    with open(ROUTES_JSON, 'w') as f:
        f.write('{"answers": [\n' + ',\n'.join(json.dumps(t) for t in route_triples()) + '\n]}\n')
    print(f'wrote {ROUTES_JSON}')
