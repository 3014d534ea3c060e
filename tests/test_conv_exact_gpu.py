"""mcgen_conv_fused against the exact float64 reference of tests/conv_exact_ref.py, route by route and switch by switch.

Inputs are small dyadic rationals on which every partial sum of the kernels' fp32 arithmetic is exact (conv_exact_ref's
docstring; `assert_exact` checks the condition per case from the reference alone).  An fp32 launch must therefore EQUAL
the reference, a bf16 launch its round-to-nearest-even to bf16, bit for bit: one wrong term anywhere -- a tap at a tile
seam, a chunk edge of the second segment, one image of a pair, a switch a route accepts but does not implement, two
epilogue steps in the wrong order -- fails at any magnitude.

Per (case, option) pair of conv_exact_ref.BASE_CASES x SWEEP and MODE_CASES x their options:
  * the plan's answer equals the one tests/golden/conv_exact_routes.json pins (route and, where the plan reports one, tile);
  * where the plan refuses, the launch refuses with the same text and nothing runs;
  * otherwise the output equals the reference (gathered / permuted where the output is compacted), padding channels
    are exactly zero, and a paired layout leaves the caller's halves alone;
  * statistics partials, summed over tiles in float64: the column sum of v is exact (equality); the second sum
    (v * xhat / v * v, whose products are not fp32 numbers) is within n 2^-24 sum|term|, n the pixels per column -- the
    fp32 summation bound;
  * with tanh_out the pre-activation is exact and the only error is the device tanhf: the test measures
    E = max |tanh_f32(v) - tanh_f64(v)| on its own v with torch.tanh on a float32 device tensor (not code under test)
    and allows 2 E plus half an ulp of the output type.  Measured on the MI355X over all tanh pairs of the tables:
    E = 5.5e-8 (the test prints it per pair).

No form rounds twice: every epilogue here stages fp32 through LDS, so no pair gets a two-rounding bound.
"""
import ctypes as C
import json
import os
import zlib

import pytest
import torch

import conv_exact_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'conv_exact_routes.json')) as _f:
    PINNED = {(n, o): a for n, o, a in json.load(_f)['answers']}
PAIRS = [(n, o, c) for n, o, c in R.pairs() if c is not None]
SENTINEL = 3.0


def _ops():
    from mcgen_amd import ops
    return ops


def _sync():
    """Wait for the launch; a device-side fault ends the whole session -- nothing more is launched on a faulted GPU."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault, stopping the session: {e}', returncode=3)


def _cidx(cm, c, cap):
    """the active channels of every image in order, padded with c: the cidx part of mcgen_mc_cmap's records"""
    return cm[:, c:c + cap].long()


def _gather_last(x, idx):
    """x[n, ..., idx[n, j]] with index == x.shape[-1] reading zero"""
    xp = torch.nn.functional.pad(x, (0, 1))
    shape = (x.shape[0],) + (1,) * (x.dim() - 2) + (idx.shape[1],)
    return torch.gather(xp, x.dim() - 1, idx.view(shape).expand(x.shape[:-1] + (idx.shape[1],))).contiguous()


def _device_buffers(ops, c, t, dtype):
    """The launch's buffers from the float64 tensors of the case: activations in `dtype` (exact: at most 8 significant
    bits), parameters in fp32, the weight image(s) through the library's own builders."""
    n, co, cy = c['N'], c['Cout'], c['Cy']
    b, extra = {}, {}
    images = []                                                      # per weight set: the segments' images in order
    sets = c['wsel'] or 1
    perm = None
    if c['yperm']:
        perm = torch.argsort((t['ycode'] == 0).to(torch.int8), dim=1, stable=True)         # [sets, Cout]: active channels first
        b['yperm'] = perm.to(torch.int16).contiguous()
        extra['perm'] = perm
    for i, s in enumerate(c['segs']):
        x = t[f'x{i}']
        cw = s['Cw'] or s['C']
        code = t.get(f'code{i}')
        if s['cmap']:
            cm = ops.mc_cmap(code.float().contiguous())
            b[f'cmap{i}'] = cm
        if c['w_layout'] == 2 and s['cmap']:
            # the producer stored the active channels only: x compacted through the map, the affine and the code as per-image rows
            idx = _cidx(cm, cw, s['C'])
            x = _gather_last(x, idx)
            sc = t[f'scale{i}'] if s['affine'] else torch.ones(cw, dtype=torch.float64, device=x.device)
            sh = t[f'shift{i}'] if s['affine'] else torch.zeros(cw, dtype=torch.float64, device=x.device)
            if sc.dim() == 2:                                        # BatchNorm groups: image n takes row n / group_n
                sc, sh = sc.repeat_interleave(s['group_n'], 0), sh.repeat_interleave(s['group_n'], 0)
            code = code if code is not None else torch.ones_like(x[:, 0, 0, :])
            b[f'scale{i}'] = _gather_last(sc * code, idx).float()
            b[f'shift{i}'] = _gather_last(sh * code, idx).float()
        else:
            if s['affine']:
                b[f'scale{i}'], b[f'shift{i}'] = t[f'scale{i}'].float().contiguous(), t[f'shift{i}'].float().contiguous()
            if s['code']:
                b[f'code{i}'] = code.float().contiguous()
        b[f'x{i}'] = x.to(dtype).contiguous()
        w = t[f'w{i}'].float()
        w = w if c['wsel'] else w[None]
        per_set = []
        for k in range(sets):
            wk = w[k][perm[k]] if perm is not None else w[k]
            per_set.append(ops.prep_weight_k(wk.contiguous(), dtype) if c['w_layout'] else ops.prep_weight(wk.contiguous(), dtype))
        images.append(per_set)
    b['w'] = torch.cat([images[i][k] for k in range(sets) for i in range(len(c['segs']))])
    for k in ('bias', 'bias2', 'gscale', 'gshift', 'gmean', 'grstd', 'ocode'):
        if k in t:
            b[k] = t[k].float().contiguous()
    ho, wo = (c['H'] >> 1, c['W'] >> 1) if c['pool'] else (c['H'], c['W'])
    for k in ('gate_x', 'res'):
        if k in t:
            b[k] = torch.nn.functional.pad(t[k], (0, cy - co)).to(dtype).contiguous()
    if c['wsel']:
        sel = t['wsel']
        if c['order']:
            b['order'] = t['order'].to(torch.int32).contiguous()
            sel = sel[t['order']]                                   # wsel is indexed by POSITION in the walk
        b['wsel'] = sel.to(torch.int32).contiguous()
    if c['ycmap']:
        cp = R.pad8(co)
        b['ycmap'] = ops.mc_cmap(torch.nn.functional.pad(t['ycode'], (0, cp - co)).float().contiguous())
        extra['yidx'] = _cidx(b['ycmap'], cp, cy)
    imgs = 2 * n if c['y_group'] else n
    b['y'] = torch.full((imgs, ho, wo, cy), SENTINEL, dtype=dtype, device='cuda')
    return b, extra


def _expected_out(c, ref_v, dtype, extra, t):
    """what y must hold, [N, Ho, Wo, Cy], from the reference's (rounded) dense result"""
    co, cy = c['Cout'], c['Cy']
    if c['ycmap']:
        idx = extra['yidx'].clamp(max=co)                            # (the zero row's index, C rounded up to 8 -> the padded column)
        return _gather_last(ref_v, idx)
    if c['yperm']:
        idx = extra['perm'][t['wsel']][:, :cy]
        return _gather_last(ref_v, idx)
    return torch.nn.functional.pad(ref_v, (0, cy - co))


TANH_E_SEEN = [0.0]


@pytest.mark.parametrize('name,option,c', PAIRS, ids=[f'{n}-{o}' for n, o, _ in PAIRS])
def test_conv_exact(name, option, c):
    from mcgen_amd import _lib
    ops, lib = _ops(), _lib.load()
    dtype = torch.bfloat16 if c['dtype'] == 'bf16' else torch.float32
    answer = R.answer(c)
    assert answer == PINNED[(name, option)], (answer, PINNED[(name, option)])
    gen = torch.Generator(device='cuda').manual_seed(zlib.crc32(f'{name}/{option}'.encode()))
    t = R.exact_inputs(gen, c)
    b, extra = _device_buffers(ops, c, t, dtype)
    p = R.descriptor(c, ptr=lambda k: b[k].data_ptr())
    plan = _lib.ConvPlan()
    rc = lib.mcgen_conv_plan(C.byref(p), R.dtype_code(c), C.byref(plan))
    if answer.startswith('refused'):
        # the launch refuses with the plan's text and runs nothing
        assert rc != 0 and 'refused: ' + lib.mcgen_last_error().decode() == answer
        dummy = torch.zeros(16, device='cuda')
        p.stats = dummy.data_ptr()
        assert lib.mcgen_conv_fused(C.byref(p), R.dtype_code(c), torch.cuda.current_stream().cuda_stream) != 0
        assert 'refused: ' + lib.mcgen_last_error().decode() == answer
        _sync()
        assert bool((b['y'].float() == SENTINEL).all())
        return
    assert rc == 0, lib.mcgen_last_error()
    ref = R.conv_ref(c, t)
    R.assert_exact(ref['bits'], f'{name} / {option}')
    compact = bool(c['ycmap'] or c['yperm'])
    spitch = R.pad16(c['Cout']) if compact else c['Cy']
    stats = None
    if c['stats_mode']:
        stats = torch.full((plan.m_tiles, 2, spitch), float('nan'), dtype=torch.float32, device='cuda')
        p.stats = stats.data_ptr()
    assert lib.mcgen_conv_fused(C.byref(p), R.dtype_code(c), torch.cuda.current_stream().cuda_stream) == 0, lib.mcgen_last_error()
    _sync()

    n, co, cy = c['N'], c['Cout'], c['Cy']
    y = b['y']
    if c['y_group']:
        g = c['y_group']
        y = y.view(n // g, 2, g, *y.shape[1:])
        assert bool((y[:, 0].float() == SENTINEL).all()), 'the paired layout wrote into the caller\'s halves'
        y = y[:, 1].reshape(n, *y.shape[3:])
    pix = n * y.shape[1] * y.shape[2]
    half_ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -24            # relative, of the stored value
    if c['tanh_out']:
        e = float((torch.tanh(ref['pre'].float()).double() - ref['v']).abs().max())
        TANH_E_SEEN[0] = max(TANH_E_SEEN[0], e)
        print(f'tanh: E = {e:.3e} (largest so far {TANH_E_SEEN[0]:.3e})')
        err = (y[..., :co].double() - ref['v']).abs()
        tol = 2 * e + half_ulp * ref['v'].abs() + 2.0 ** -133
        assert bool((err <= tol).all()), f'tanh output: max err {float(err.max()):.3e}, E {e:.3e}'
        assert bool((y[..., co:].float() == 0).all())
    else:
        want = _expected_out(c, R.round_out(ref['v'], dtype), dtype, extra, t)
        if not torch.equal(y, want):
            bad = (y.float() != want.float())
            where = torch.nonzero(bad)[:5].tolist()
            raise AssertionError(f'{int(bad.sum())} of {bad.numel()} outputs differ from the exact result; first at (n, h, w, c) = {where}: '
                                 f'got {y[bad][:5].tolist()}, want {want[bad][:5].tolist()}')
    if stats is not None:
        s = stats.double().sum(0)[:, :co]
        s0, s1 = ref['sums']
        a0, a1 = ref['sums_abs']
        eps = 2.0 ** -24
        if c['tanh_out']:
            # every term carries the tanh error: <= 2 E per v, <= 2 * 2 E per v * v (|v| <= 1)
            assert bool(((s[0] - s0).abs() <= pix * eps * a0 + pix * 2 * e).all()), (s[0] - s0).abs().max()
            assert bool(((s[1] - s1).abs() <= pix * eps * a1 + pix * 4 * e).all()), (s[1] - s1).abs().max()
        else:
            assert torch.equal(s[0], s0), f'column sums of v: max diff {float((s[0] - s0).abs().max()):.3e}'
            assert bool(((s[1] - s1).abs() <= pix * eps * a1).all()), \
                f'second sums: max diff {float((s[1] - s1).abs().max()):.3e}, bound {float((pix * eps * a1).min()):.3e}'
