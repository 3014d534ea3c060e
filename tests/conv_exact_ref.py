"""Exact float64 references of mcgen_conv_fused and of the weight-gradient kernels, and inputs on which the kernels'
own fp32 arithmetic is exact (tests/test_conv_exact_ref_cpu.py, test_conv_exact_gpu.py, test_wgrad_exact_gpu.py).

The idea.  Every operand is a small dyadic rational: activations, residuals, gate inputs and output gradients are
multiples of 1/4, BatchNorm-like scales are 0.5 / 1 / 2, shifts and biases multiples of 1/4, weights multiples of 1/8 in
[-1/2, 1/2], MultimodalController codes 0 / 0.5 / 1 / 2.  A prologue result is then a multiple of 1/16 below 16 (8
significant bits: exact in bf16, which is what the bf16 kernels stage into LDS), every product is a multiple of a common
quantum q, and as long as  sum |term| < 2^24 q  EVERY partial sum -- whatever the order, the split over waves, K parts,
tiles or slabs -- is an integer multiple of q below 2^24 q, i.e. an fp32 number.  The fp32 accumulators then hold the
mathematical result: an fp32 launch must equal the float64 reference bit for bit, a bf16 launch its round-to-nearest-even
to bf16.  `assert_exact` checks the condition from the reference alone.

The contract is read from include/mcgen_hip.h (mcgen_seg_t, mcgen_conv_t, mcgen_wgrad_t), not from a kernel:
    prologue per segment   a = x[n, h >> ups, w >> ups, c];  a = a * scale[row][c] + shift[row][c] (row = n / group_n);
                           a = max(a, 0);  a = a * code[n, c];   the convolution's zero padding comes AFTER this
    acc                    sum over segments of conv(a, W) (3x3 pad 1 / 1x1), 2x2 window sums when pool
    epilogue on v = alpha * acc:  + (bias + bias2);  * ocode[n, co];  * (gate_x * gscale + gshift > 0);
                           stats_mode 2 sums v and v * xhat;  + res;  tanh;  stats_mode 1 sums v and v * v

Everything here is NHWC float64 torch on whatever device the inputs live on; the only project import is the ctypes
structure a descriptor needs.

A case is a dict of SHAPE and OPTION fields only:
    name, dtype ('bf16' / 'f32'), N, H, W (convolution resolution), Cout, Cy (default: Cout rounded up to 8),
    segs: [{C, ksize (3), ups, relu, affine, code, group_n, cmap, Cw}],
    bias (1), bias2, alpha (1.0), ocode, gate (1: plain ReLU gate, 2: with gscale / gshift), stats_mode, res, tanh_out,
    pool, w_layout, ycmap, wsel (number of weight sets), order, yperm, y_group, xr (value range of x in quarters)
"""
import copy
import ctypes as C
import math

import torch
import torch.nn.functional as F

from mcgen_amd import _lib            # the ctypes structures and mcgen_cmap_stride: what a descriptor needs

DUMMY = 0x1000
ROUTES = ('tiled', 'mc', 'gk', 'gk-pp', 'skinny', 'smap', 'px1', 'c8', 'head')
SEG_DEFAULTS = dict(ksize=3, ups=0, relu=0, affine=0, code=0, group_n=0, cmap=0, Cw=0)
CASE_DEFAULTS = dict(dtype='bf16', bias=1, bias2=0, alpha=1.0, ocode=0, gate=0, stats_mode=0, res=0, tanh_out=0, pool=0,
                     w_layout=0, ycmap=0, wsel=0, order=0, yperm=0, y_group=0, xr=4)
STATS_TILE = 256            # the largest pixel tile any route sums into one row of `stats`


def pad8(c):
    return (c + 7) // 8 * 8


def pad16(c):
    return (c + 15) // 16 * 16


def full(case):
    """The case with every default written out (a deep copy)."""
    c = dict(CASE_DEFAULTS)
    c.update(copy.deepcopy(case))
    c['segs'] = [dict(SEG_DEFAULTS, **s) for s in c['segs']]
    c.setdefault('Cy', pad8(c['Cout']))
    return c


# ---- the options: each a function case -> case (or None where the base cannot take it) ---------------------------------
def _seg0(**kw):
    def f(c):
        c['segs'][0].update(kw)
        return c
    return f


def _top(**kw):
    def f(c):
        c.update(kw)
        return c
    return f


def _group(c):
    n = c['N']
    c['segs'][0].update(affine=1, group_n=n // 2 if n % 2 == 0 and n >= 4 else n)
    return c


def _seg2(**kw):
    def f(c):
        if len(c['segs']) != 1:
            return None
        c['segs'].append(dict(SEG_DEFAULTS, C=c.get('seg2_C', 16), **kw))
        return c
    return f


def _pool(**kw):
    def f(c):
        if c['H'] < 2 or c['W'] < 2:
            return None
        c.update(pool=1, alpha=0.25, **kw)
        return c
    return f


OPTIONS = {
    'base': lambda c: c,
    # prologue and segments
    'affine': _seg0(affine=1), 'relu': _seg0(relu=1), 'code': _seg0(code=1), 'affine+relu+code': _seg0(affine=1, relu=1, code=1),
    'ups': _seg0(ups=1), 'group_n': _group, 'seg2': _seg2(ksize=1), 'seg2ups': _seg2(ksize=1, ups=1),
    'seg2k3': _seg2(ksize=3, affine=1, relu=1, code=1),
    # epilogue
    'alpha': _top(alpha=0.5), 'nobias': _top(bias=0), 'bias2': _top(bias2=1), 'ocode': _top(ocode=1), 'gate': _top(gate=1),
    'gate_bn': _top(gate=2), 'stats1': _top(stats_mode=1), 'stats2': _top(stats_mode=2, gate=2), 'res': _top(res=1),
    'tanh': _top(tanh_out=1), 'pool': _pool(), 'pool+res': _pool(res=1),
    # the two orders a single option cannot tell apart: the backward sums exclude `res` and include the code and the gate;
    # the forward sums see the residual and the tanh
    'order_bwd': _top(ocode=1, gate=2, stats_mode=2, res=1),
    'order_fwd': _top(bias=1, bias2=1, res=1, tanh_out=1, stats_mode=1),
    # the same neighbours for the routes that take neither gscale nor tanh (the whole-image kernel): code, plain gate,
    # residual, and the forward sums behind all three
    'order_gate_res': _top(ocode=1, gate=1, res=1, stats_mode=1),
}


def apply_option(base, name):
    """The full case of (base, option), or None where the option does not apply to the base's shape."""
    c = OPTIONS[name](full(base))
    if c is None:
        return None
    if any(s['ups'] for s in c['segs']) and (c['H'] < 2 or c['W'] < 2):       # (no tensor of half the resolution exists)
        return None
    return c


# ---- the descriptor -----------------------------------------------------------------------------------------------------
def descriptor(case, ptr=None):
    """mcgen_conv_t of a case from its shape and option fields.  `ptr(name)` gives the address of
    a buffer ('x0', 'scale0', ..., 'w', 'bias', ...); without it every buffer the case uses is the dummy address 0x1000,
    which mcgen_conv_plan never dereferences.  `stats` stays NULL: the plan must not need it."""
    c = full(case)
    at = ptr if ptr is not None else (lambda name: DUMMY)
    p = _lib.Conv()
    p.nseg = len(c['segs'])
    for i, s in enumerate(c['segs']):
        g = p.seg[i]
        g.x = at(f'x{i}')
        mapped = bool(s['cmap'])
        gk_rows = c['w_layout'] == 2 and mapped           # w_layout 2: the code of a compacted segment rides in per-image rows
        has_aff = bool(s['affine']) or (gk_rows and bool(s['code']))
        g.scale = at(f'scale{i}') if has_aff else None
        g.shift = at(f'shift{i}') if has_aff else None
        g.code = at(f'code{i}') if s['code'] and not gk_rows else None
        g.cmap = at(f'cmap{i}') if mapped else None
        g.C, g.ups, g.relu, g.ksize = s['C'], s['ups'], s['relu'], s['ksize']
        g.group_n = 1 if gk_rows and has_aff else s['group_n']
        g.Cw = s['Cw']
        g.cmap_stride = cmap_stride(s['Cw'] or s['C']) if mapped else 0
    p.w, p.y = at('w'), at('y')
    p.bias = at('bias') if c['bias'] else None
    p.bias2 = at('bias2') if c['bias2'] else None
    p.res = at('res') if c['res'] else None
    p.ocode = at('ocode') if c['ocode'] else None
    p.gate_x = at('gate_x') if c['gate'] else None
    p.gscale = at('gscale') if c['gate'] == 2 else None
    p.gshift = at('gshift') if c['gate'] == 2 else None
    p.gmean = at('gmean') if c['stats_mode'] == 2 else None
    p.grstd = at('grstd') if c['stats_mode'] == 2 else None
    p.N, p.H, p.W = c['N'], c['H'], c['W']
    p.Cout, p.Cout_w, p.Cy = c['Cout'], pad16(c['Cout']), c['Cy']
    p.pool, p.alpha, p.tanh_out, p.stats_mode = c['pool'], c['alpha'], c['tanh_out'], c['stats_mode']
    p.w_layout, p.y_group = c['w_layout'], c['y_group']
    if c['ycmap']:
        p.ycmap, p.ycmap_stride = at('ycmap'), cmap_stride(pad8(c['Cout']))
    if c['wsel']:
        p.wsel, p.wsel_stride = at('wsel'), weight_elems(c)
    if c['order']:
        p.order = at('order')
    if c['yperm']:
        p.yperm, p.yperm_stride = at('yperm'), c['Cout']
    return p


def cmap_stride(c):
    """int16 elements of one record of mcgen_mc_cmap over c channels (a host-side query)"""
    return int(_lib.load().mcgen_cmap_stride(c))


def weight_elems(case):
    """elements of ONE chunked weight image of the case ([chunk][tap][Cout_w][32] per segment, segments in order)."""
    return sum(((s['C'] + 31) // 32) * s['ksize'] ** 2 for s in case['segs']) * pad16(case['Cout']) * 32


def dtype_code(case):
    return _lib.BF16 if case.get('dtype', 'bf16') == 'bf16' else _lib.F32


def plan(case):
    """(rc, error text, plan fields) of mcgen_conv_plan for the case's descriptor (no HIP call: answers without a GPU)."""
    lib = _lib.load()
    p = descriptor(case)
    out = _lib.ConvPlan()
    rc = lib.mcgen_conv_plan(C.byref(p), dtype_code(case), C.byref(out))
    if rc:
        return rc, lib.mcgen_last_error().decode(), None
    return 0, None, {k: getattr(out, k) for k in ('route', 'form', 'bm', 'bn', 'pipe', 'm_tiles', 'grouped')}


def answer(case):
    """The plan's answer as one string: 'refused: <text>' or the instantiation 'route[/bm x bn/pipe][/g]'."""
    rc, err, pl = plan(case)
    if rc:
        return 'refused: ' + err
    s = ROUTES[pl['route']]
    if pl['bm']:
        s += f"/{pl['bm']}x{pl['bn']}/{pl['pipe']}"
    if pl['grouped']:
        s += '/g'
    return s


# ---- inputs on the dyadic grid ------------------------------------------------------------------------------------------
def _quarters(gen, shape, r):
    return torch.randint(-r, r + 1, shape, generator=gen, device=gen.device).double() / 4


def _pick(gen, shape, values):
    v = torch.tensor(values, dtype=torch.float64, device=gen.device)
    return v[torch.randint(0, len(values), shape, generator=gen, device=gen.device)]


def exact_inputs(gen, case):
    """Float64 tensors (NHWC, on the generator's device) of a case on the dyadic grid of the module docstring:
    x{i}, scale{i}, shift{i} ([groups, C] with group_n, else [C]), code{i} [N, C], w{i} [Cout, C, k, k] ([sets, Cout, C, k, k]
    with wsel), bias, bias2, ocode [N, Cout], gate_x / res [N, Ho, Wo, Cout], gscale, gshift, gmean, grstd [Cout],
    wsel [N] (int64), order [N] (a permutation), ycode [N, Cout] (the consumer's code of a compacted output)."""
    c = full(case)
    n, h, w, co = c['N'], c['H'], c['W'], c['Cout']
    t = {}
    for i, s in enumerate(c['segs']):
        hs, ws = (h >> 1, w >> 1) if s['ups'] else (h, w)
        cs = s['Cw'] or s['C']                            # (w_layout 2: the TRUE channels; the test compacts them)
        t[f'x{i}'] = _quarters(gen, (n, hs, ws, cs), c['xr'])
        if s['affine']:
            rows = (n // s['group_n'],) if s['group_n'] else ()
            t[f'scale{i}'] = _pick(gen, rows + (cs,), [0.5, 1.0, 2.0])
            t[f'shift{i}'] = _quarters(gen, rows + (cs,), 4)
        if s['code']:
            t[f'code{i}'] = _pick(gen, (n, cs), [0.0, 0.0, 0.5, 1.0, 2.0])
            if n > 2 and s['cmap']:                        # an image with no active channel, one with all of them
                t[f'code{i}'][0] = 0.0
                t[f'code{i}'][1] = 1.0
            if s['Cw']:                                   # compacted storage: at most C active channels per image, one image with exactly C
                cd = t[f'code{i}']
                cd[1, s['C']:] = 0.0
                cd *= ((cd != 0).cumsum(1) <= s['C'])
        sets = (c['wsel'],) if c['wsel'] else ()
        t[f'w{i}'] = torch.randint(-4, 5, sets + (co, cs, s['ksize'], s['ksize']), generator=gen, device=gen.device).double() / 8
    ho, wo = (h >> 1, w >> 1) if c['pool'] else (h, w)
    if c['bias']:
        t['bias'] = _quarters(gen, (co,), 8)
    if c['bias2']:
        t['bias2'] = _quarters(gen, (co,), 8)
    if c['ocode']:
        t['ocode'] = _pick(gen, (n, co), [0.0, 0.5, 1.0, 2.0])
    if c['gate']:
        t['gate_x'] = _quarters(gen, (n, ho, wo, co), 4)
    if c['gate'] == 2:
        t['gscale'] = _pick(gen, (co,), [0.5, 1.0, 2.0])
        t['gshift'] = _quarters(gen, (co,), 2)
    if c['stats_mode'] == 2:
        t['gmean'] = _quarters(gen, (co,), 2)
        t['grstd'] = _pick(gen, (co,), [0.5, 1.0, 2.0])
    if c['res']:
        t['res'] = _quarters(gen, (n, ho, wo, co), 8)
    if c['wsel']:
        t['wsel'] = torch.randint(0, c['wsel'], (n,), generator=gen, device=gen.device)
    if c['order']:
        t['order'] = torch.randperm(n, generator=gen, device=gen.device)
    if c['ycmap'] or c['yperm']:
        # the consumer's 0 / 1 code: per image (ycmap) or per weight set (yperm); at most Cy active channels, rows with none
        # and with exactly Cy among them
        rows = c['wsel'] if c['yperm'] else n
        cap = min(c['Cy'], co)
        cnt = torch.randint(0, cap + 1, (rows,), generator=gen, device=gen.device)
        cnt[0], cnt[-1] = cap, 0
        rank = torch.rand((rows, co), generator=gen, device=gen.device).argsort(1).argsort(1)
        t['ycode'] = (rank < cnt[:, None]).double()
    return t


def real_inputs(gen, case):
    """The same tensors with Gaussian (non-dyadic) values: the reference checked as mathematics against torch."""
    t = exact_inputs(gen, case)
    for k, v in t.items():
        if v.dtype == torch.float64 and not k.startswith('ycode'):
            r = torch.randn(v.shape, generator=gen, dtype=torch.float64, device=gen.device)
            t[k] = r.abs() + 0.25 if k == 'grstd' else r * (0.2 if k[0] == 'w' else 1.0)
    return t


# ---- the reference ------------------------------------------------------------------------------------------------------
def prologue(x, scale, shift, relu, code, ups, group_n):
    """mcgen_seg_t's prologue on an NHWC tensor: upsample, affine (row n / group_n), ReLU, code."""
    n = x.shape[0]
    if ups:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    if scale is not None:
        if group_n > 0:
            rows = torch.arange(n, device=x.device) // group_n
            x = x * scale[rows][:, None, None, :] + shift[rows][:, None, None, :]
        else:
            x = x * scale + shift
    if relu:
        x = x.clamp_min(0)
    if code is not None:
        x = x * code[:, None, None, :]
    return x


def conv_nhwc(a, w, chunk=16):
    """sum_{kh, kw, ci} a[n, h + kh - pad, w + kw - pad, ci] * w[co, ci, kh, kw] with zero padding, as tap-wise matmuls."""
    k = w.shape[-1]
    n, h, wd, _ = a.shape
    ap = F.pad(a, (0, 0, k // 2, k // 2, k // 2, k // 2))
    out = torch.zeros((n, h, wd, w.shape[0]), dtype=a.dtype, device=a.device)
    for i0 in range(0, n, chunk):
        for dh in range(k):
            for dw in range(k):
                out[i0:i0 + chunk] += ap[i0:i0 + chunk, dh:dh + h, dw:dw + wd, :] @ w[:, :, dh, dw].t()
    return out


def _conv_sets(a, w, sel):
    if w.dim() == 4:
        return conv_nhwc(a, w)
    out = torch.zeros(a.shape[:3] + (w.shape[1],), dtype=a.dtype, device=a.device)
    for s in range(w.shape[0]):
        idx = torch.nonzero(sel == s).flatten()
        if idx.numel():
            out[idx] = conv_nhwc(a[idx], w[s])
    return out


def _pool2(x):
    return x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]


def _quantum(*ts):
    """the largest power of two <= 1 that divides every entry of the tensors"""
    k = 0
    for t in ts:
        t = t.reshape(-1)
        while k < 60 and not bool((t * 2.0 ** k == torch.round(t * 2.0 ** k)).all()):
            k += 1
    return 2.0 ** -k


def _bits(mag, q):
    """mantissa bits of an integer multiple of q of magnitude <= mag"""
    return 0 if mag <= 0 else int(math.floor(math.log2(mag / q))) + 1


def conv_ref(case, t, want_S=True):
    """Float64 restatement of mcgen_conv_fused for `case` on the tensors `t` (exact_inputs / real_inputs, any device).
    Returns a dict:
        v      [N, Ho, Wo, Cout]  the value before output rounding
        pre    the argument of tanh (== v without tanh_out)
        sums   None, or (sum0 [Cout], sum1 [Cout]): column sums of v and v * xhat (stats_mode 2, taken in front of `res`)
               or of v and v * v (stats_mode 1, taken last), and
        sums_abs  (sum |v|, sum |second term|) for the fp32 summation bound
        S      conv(|a|, |w|) |alpha| + |bias| + |bias2|, times |ocode|, + |res|: bounds |v| and every partial sum
        bits   the most mantissa bits any partial sum of the accumulation, the epilogue or a tile's column sum of v needs
    """
    c = full(case)
    acc, S, q_acc = 0, 0, 1.0
    for i, s in enumerate(c['segs']):
        a = prologue(t[f'x{i}'], t.get(f'scale{i}'), t.get(f'shift{i}'), s['relu'], t.get(f'code{i}'), s['ups'], s['group_n'])
        w = t[f'w{i}']
        acc = acc + _conv_sets(a, w, t.get('wsel'))
        if want_S:
            S = S + _conv_sets(a.abs(), w.abs(), t.get('wsel'))
        q_acc = min(q_acc, _quantum(a) * _quantum(w))
    if c['pool']:
        acc = _pool2(acc)
        S = _pool2(S) if want_S else S
    if not want_S:
        S = acc.abs()                                         # (a lower bound: the caller did not ask for the bits of the sum)
    bits = _bits(float(S.max()), q_acc)
    alpha = c['alpha']
    b = 0
    if c['bias']:
        b = b + t['bias']
    if c['bias2']:
        b = b + t['bias2']
    v, S = alpha * acc + b, abs(alpha) * S + (b.abs() if torch.is_tensor(b) else 0)
    q = min(q_acc * _quantum(torch.tensor([alpha], dtype=torch.float64)), _quantum(b) if torch.is_tensor(b) else 1.0)
    bits = max(bits, _bits(float(S.max()), q))
    if c['ocode']:
        oc = t['ocode'][:, None, None, :]
        v, S, q = v * oc, S * oc.abs(), q * _quantum(t['ocode'])
        bits = max(bits, _bits(float(S.max()), q))
    sums = sums_abs = None
    if c['gate']:
        z = t['gate_x'] * t['gscale'] + t['gshift'] if c['gate'] == 2 else t['gate_x']
        v = v * (z > 0)
    if c['stats_mode'] == 2:
        xhat = (t['gate_x'] - t['gmean']) * t['grstd']
        sums = (v.sum((0, 1, 2)), (v * xhat).sum((0, 1, 2)))
        sums_abs = (v.abs().sum((0, 1, 2)), (v * xhat).abs().sum((0, 1, 2)))
        bits = max(bits, _bits(STATS_TILE * float(v.abs().max()), q))
    if c['res']:
        v, S, q = v + t['res'], S + t['res'].abs(), min(q, _quantum(t['res']))
        bits = max(bits, _bits(float(S.max()), q))
    pre = v
    if c['tanh_out']:
        v = torch.tanh(v)
    if c['stats_mode'] == 1:
        sums = (v.sum((0, 1, 2)), (v * v).sum((0, 1, 2)))
        sums_abs = (v.abs().sum((0, 1, 2)), (v * v).sum((0, 1, 2)))
        if not c['tanh_out']:
            bits = max(bits, _bits(STATS_TILE * float(v.abs().max()), q))
    return dict(v=v, pre=pre, sums=sums, sums_abs=sums_abs, S=S, bits=bits, q=q)


def bound_bits(case, t):
    """An upper bound of conv_ref's accumulation / epilogue bits without a convolution: |a| and |w| by their maxima, K by its
    count.  What the CPU test can afford for every case of the tables; it never reports fewer bits than conv_ref's `S`."""
    c = full(case)
    S, q = 0.0, 1.0
    for i, s in enumerate(c['segs']):
        a = prologue(t[f'x{i}'], t.get(f'scale{i}'), t.get(f'shift{i}'), s['relu'], t.get(f'code{i}'), s['ups'], s['group_n'])
        w = t[f'w{i}']
        S += s['ksize'] ** 2 * a.shape[-1] * float(a.abs().max()) * float(w.abs().max())
        q = min(q, _quantum(a) * _quantum(w))
    if c['pool']:
        S *= 4
    bits = _bits(S, q)
    b = sum(float(t[k].abs().max()) for k in ('bias', 'bias2') if k in t)
    S = abs(c['alpha']) * S + b
    q = min(q * _quantum(torch.tensor([c['alpha']], dtype=torch.float64)), *[_quantum(t[k]) for k in ('bias', 'bias2') if k in t], 1.0)
    bits = max(bits, _bits(S, q))
    if c['ocode']:
        S, q = S * float(t['ocode'].abs().max()), q * _quantum(t['ocode'])
        bits = max(bits, _bits(S, q))
    if c['res']:
        S, q = S + float(t['res'].abs().max()), min(q, _quantum(t['res']))
        bits = max(bits, _bits(S, q))
    return bits


def assert_exact(bits, what=''):
    """The condition on the INPUTS under which fp32 arithmetic is exact: every partial sum fits fp32's 24-bit significand.
    A case that breaks it is a broken case (shrink its value range), never a tolerance to widen."""
    assert bits <= 24, f'{what}: a partial sum can need {bits} bits: the inputs are too large for exact fp32 sums'


def round_out(v, dtype):
    """what an exact launch stores: the value itself in fp32, its round-to-nearest-even in bf16"""
    v = v.float()
    return v if dtype == torch.float32 else v.bfloat16()


# ---- weight gradients ---------------------------------------------------------------------------------------------------
def wgrad_inputs(gen, n, h, w, cin, cout, ksize, ups=0, dy_ups=0, prologue_on=0, xr=4):
    """x [N, H >> ups, W >> ups, Cin], dy [N, H >> dy_ups, W >> dy_ups, Cout] in quarters; with `prologue_on` the triple
    (scale, shift, ReLU, a code from {0, 0.5, 1, 2}); grad0 / bias0: dyadic initial gradients for accumulate."""
    t = {'x': _quarters(gen, (n, h >> ups, w >> ups, cin), xr), 'dy': _quarters(gen, (n, h >> dy_ups, w >> dy_ups, cout), 4)}
    if prologue_on:
        t['scale'], t['shift'] = _pick(gen, (cin,), [0.5, 1.0, 2.0]), _quarters(gen, (cin,), 4)
        t['code'] = _pick(gen, (n, cin), [0.0, 0.5, 1.0, 2.0])
    t['grad0'] = _quarters(gen, (cout, cin, ksize, ksize), 16)
    t['bias0'] = _quarters(gen, (cout,), 16)
    return t


def wgrad_ref(t, ksize, ups=0, dy_ups=0, relu=0, alpha=1.0):
    """dW[co, ci, kh, kw] = alpha * sum_{n, h, w} dy[n, (h, w) >> dy_ups, co] * prologue(x)[n, h + kh - pad, w + kw - pad, ci]
    and the bias gradient alpha * sum dy (every pixel of the convolution's resolution), in float64.
    Returns (dW [Cout, Cin, k, k], dbias [Cout], bits): bits as in conv_ref, for the sums over ALL pixels (slabs and their
    reduction included)."""
    a = prologue(t['x'], t.get('scale'), t.get('shift'), relu, t.get('code'), ups, 0)
    dy = t['dy']
    if dy_ups:
        dy = dy.repeat_interleave(2, 1).repeat_interleave(2, 2)
    n, h, w, cin = a.shape
    k = ksize
    ap = F.pad(a, (0, 0, k // 2, k // 2, k // 2, k // 2))
    dw = torch.zeros((dy.shape[-1], cin, k, k), dtype=torch.float64, device=a.device)
    s_abs = 0.0
    d2 = dy.reshape(-1, dy.shape[-1])
    for kh in range(k):
        for kw in range(k):
            win = ap[:, kh:kh + h, kw:kw + w, :].reshape(-1, cin)
            dw[:, :, kh, kw] = d2.t() @ win
            s_abs = max(s_abs, float((d2.abs().t() @ win.abs()).max()))
    db = d2.sum(0)
    qa = _quantum(torch.tensor([alpha], dtype=torch.float64))
    q = _quantum(a) * _quantum(dy)
    bits = max(_bits(s_abs, q), _bits(abs(alpha) * s_abs + float(t['grad0'].abs().max()), min(q * qa, _quantum(t['grad0']))),
               _bits(abs(alpha) * float(d2.abs().sum(0).max()) + float(t['bias0'].abs().max()), min(_quantum(dy) * qa, _quantum(t['bias0']))))
    return alpha * dw, alpha * db, bits


# ---- the tables ---------------------------------------------------------------------------------------------------------
def _case(name, n, h, w, cout, segs, **kw):
    return dict(name=name, N=n, H=h, W=w, Cout=cout, segs=segs, **kw)


def _s(c, **kw):
    return dict(C=c, **kw)


# The smallest shape that reaches each instantiation (route thresholds are on pixels and Cout_w, never on K: K stays small
# unless the route demands it).  Every option of OPTIONS is toggled on each of them.
BASE_CASES = [
    # fp32 table
    _case('f32 128x16', 3, 8, 8, 3, [_s(16)], dtype='f32'),                      # odd N, Cout 3 in a pitch of 8
    _case('f32 64x64', 3, 8, 8, 20, [_s(16)], dtype='f32'),                      # ragged: 192 pixels, 20 of 64 channels
    _case('f32 64x64 8x16', 2, 8, 16, 72, [_s(8)], dtype='f32'),                 # non-square
    _case('f32 128x128', 17, 32, 32, 136, [_s(8)], dtype='f32'),                  # 17408 pixels: just past the threshold
    # bf16 table, small tiles
    _case('64x64', 3, 8, 8, 20, [_s(16)]),                                        # ragged; Cy 24 > Cout 20
    _case('64x64 8x16', 2, 8, 16, 72, [_s(40)]),                                  # non-square, K not a whole chunk
    _case('64x64 4x4', 5, 4, 4, 24, [_s(16)]),                                    # four images per tile, odd N
    _case('64x64 1x1 map', 5, 1, 1, 64, [_s(64, ksize=1)]),
    _case('64x16 cp', 3, 16, 16, 3, [_s(40)], Cy=16),                             # Cy 16 > Cout 3
    _case('64x16 cp 4x4', 3, 4, 4, 8, [_s(16)]),
    _case('128x16 cp', 33, 32, 32, 3, [_s(8)], Cy=16),                            # 33792 pixels
    _case('256x16', 128, 32, 32, 3, [_s(8)], Cy=16),                              # 131072 pixels; Cy 16 keeps the head away
    _case('64x128', 16, 32, 32, 136, [_s(8)]),                                     # 16384 pixels
    _case('64x64 grouped 1x1', 3, 8, 8, 24, [_s(384, ksize=1)]),                  # dma3g: 12 chunks
    # bf16 table, large tiles (65536 pixels, 32768 for 128x256)
    _case('128x64', 64, 32, 32, 24, [_s(8)]),
    _case('128x64 whole', 64, 32, 32, 64, [_s(8)]),
    _case('128x128', 64, 32, 32, 72, [_s(40)]),
    _case('128x128 whole', 64, 32, 32, 128, [_s(40)]),
    _case('256x128 pp', 64, 32, 32, 72, [_s(64)]),
    _case('256x128 pp whole', 64, 32, 32, 128, [_s(64)]),
    _case('256x128 pp W16', 256, 16, 16, 128, [_s(64)]),
    _case('128x256', 32, 32, 32, 264, [_s(40)]),
    _case('128x256 pp', 32, 32, 32, 264, [_s(64)]),
    _case('128x256 pp W16', 128, 16, 16, 264, [_s(64)]),
    _case('256x256', 64, 32, 32, 264, [_s(40)]),
    _case('256x256 pp', 64, 32, 32, 264, [_s(64)]),
    _case('256x256 pp W16', 256, 16, 16, 264, [_s(64)]),
    _case('64x16 cp W32', 3, 32, 32, 3, [_s(8)], Cy=16),
    _case('64x16 cp deep 1x1', 3, 8, 8, 12, [_s(512, ksize=1)], Cy=16),
    _case('128x128 grouped 1x1', 64, 32, 32, 72, [_s(384, ksize=1)]),
    # thin and short maps
    _case('map 16x2', 3, 16, 2, 24, [_s(16)]),
    _case('map 2x32', 3, 2, 32, 24, [_s(16)]),
    _case('map 1x16', 5, 1, 16, 24, [_s(16)]),
    _case('map 2x64', 4, 2, 64, 3, [_s(16)]),
    _case('f32 map 2x32', 3, 2, 32, 24, [_s(16)], dtype='f32'),
    _case('f32 map 2x64', 4, 2, 64, 3, [_s(16)], dtype='f32'),
    # ragged last tiles of several images each (8x8 maps, odd N) and 64-wide maps (a tile is exactly two rows)
    _case('128x64 8x8 ragged', 1025, 8, 8, 24, [_s(8)]),
    _case('128x128 8x8 ragged', 1025, 8, 8, 72, [_s(8)]),
    _case('256x256 8x8 ragged', 1025, 8, 8, 264, [_s(8)]),
    _case('256x16 8x8 ragged', 2049, 8, 8, 3, [_s(8)], Cy=16),
    _case('128x128 W64', 16, 64, 64, 72, [_s(8)]),
    _case('f32 128x128 W64', 5, 64, 64, 72, [_s(8)], dtype='f32'),
    _case('256x256 pp 16x32', 128, 16, 32, 264, [_s(64)]),
    # kernels in files of their own
    _case('skinny W4', 2, 4, 4, 3, [_s(128)]),
    _case('skinny W8', 3, 8, 8, 12, [_s(136)], Cy=16),                            # 4.25 chunks
    _case('skinny W16', 1, 16, 16, 16, [_s(128)]),
    _case('smap 128k3', 3, 8, 8, 64, [_s(128)], seg2_C=128),
    _case('smap 128k3 pair', 256, 8, 8, 128, [_s(128)], seg2_C=128),
    _case('smap 256k3', 3, 8, 8, 64, [_s(256)], seg2_C=128),
    _case('smap 256k3 pair', 256, 8, 8, 128, [_s(256)], seg2_C=128),
    _case('smap 128k1', 3, 8, 8, 128, [_s(128, ksize=1)], seg2_C=128),
    _case('smap 128k1 pair', 256, 8, 8, 128, [_s(128, ksize=1)], seg2_C=128),
    _case('smap 256k1', 3, 8, 8, 64, [_s(256, ksize=1)], seg2_C=128),
    _case('smap 256k1 pair', 256, 8, 8, 128, [_s(256, ksize=1)], seg2_C=128),
    _case('smap 256k1+128k3', 3, 8, 8, 64, [_s(256, ksize=1), _s(128)]),
    _case('smap 256k1+128k3 pair', 256, 8, 8, 128, [_s(256, ksize=1), _s(128)]),
    _case('smap 256k3+256k1ups', 3, 8, 8, 64, [_s(256), _s(256, ksize=1, ups=1)]),
    _case('smap 256k3+256k1ups pair', 256, 8, 8, 128, [_s(256), _s(256, ksize=1, ups=1)]),
    _case('px1 16x16', 3, 16, 16, 512, [_s(512, ksize=1)]),
    _case('px1 8x8', 3, 8, 8, 512, [_s(512, ksize=1)]),
    _case('px1 4x4', 3, 4, 4, 512, [_s(512, ksize=1)]),
    _case('c8 half images', 2, 32, 32, 128, [_s(8)]),
    _case('c8 whole images', 192, 32, 32, 128, [_s(8)]),
    _case('head', 3, 32, 32, 3, [_s(64)]),
]

# K-major and per-mode cases: swept over the same options (what a mode's checks do not allow is a pinned refusal) plus the
# ones named in `options`; the reference is the dense exact result, gathered where the output is compacted.
MODE_CASES = [
    _case('mc 128x128', 8, 16, 16, 128, [_s(40, affine=1, relu=1, code=1, cmap=1)], w_layout=1,
          options=['seg2mc']),
    _case('mc 128x256', 8, 16, 16, 136, [_s(40, affine=1, relu=1, code=1, cmap=1)], w_layout=1, options=[]),
    _case('mc 256x256', 64, 32, 32, 136, [_s(40, affine=1, relu=1, code=1, cmap=1, ups=1)], w_layout=1, options=['ycmap']),
    _case('gk dense 128x128', 8, 16, 16, 128, [_s(40)], w_layout=2, options=[]),
    _case('gk dense W64', 2, 64, 64, 72, [_s(8)], w_layout=2, options=[]),         # (pooling: refused, a pass holds one row)
    _case('gk 128x128', 8, 16, 16, 72, [_s(32, Cw=40, affine=1, relu=1, code=1, cmap=1)], w_layout=2, options=[]),
    _case('gk 128x256', 8, 16, 16, 136, [_s(32, Cw=40, affine=1, relu=1, code=1, cmap=1)], w_layout=2, options=[]),
    _case('mc 256x256 whole', 64, 32, 32, 264, [_s(40, affine=1, relu=1, code=1, cmap=1)], w_layout=1, options=[]),
    _case('gk 256x256', 64, 32, 32, 136, [_s(32, Cw=40, affine=1, relu=1, code=1, cmap=1)], w_layout=2, options=['ycmap']),
    _case('gk-pp', 64, 32, 32, 136, [_s(64, Cw=96, affine=1, relu=1, code=1, cmap=1)], w_layout=2, options=['ycmap']),
    _case('gk-pp whole', 64, 32, 32, 264, [_s(64, Cw=96, affine=1, relu=1, code=1, cmap=1)], w_layout=2, options=[]),
    _case('gk-pp W16', 256, 16, 16, 136, [_s(64, Cw=96, code=1, cmap=1)], w_layout=2, options=[]),
    _case('wsel', 64, 32, 32, 136, [_s(64)], wsel=3, options=['ycmap']),
    _case('wsel whole', 64, 32, 32, 264, [_s(64)], wsel=3, options=[]),
    _case('wsel + order', 64, 32, 32, 136, [_s(64)], wsel=3, order=1, options=['ycmap']),
    _case('ycmap 256x256', 64, 32, 32, 136, [_s(40)], ycmap=1, Cy=96, options=[]),
    _case('ycmap pp', 64, 32, 32, 136, [_s(64)], ycmap=1, Cy=96, options=[]),
    _case('ycmap 64x64', 4, 8, 8, 24, [_s(16)], ycmap=1, Cy=32, options=[]),
    _case('yperm 256x256', 64, 32, 32, 256, [_s(64)], wsel=3, yperm=1, Cy=160, options=[]),
    _case('yperm 256x128', 64, 32, 32, 128, [_s(64)], wsel=3, yperm=1, Cy=96, options=[]),
    _case('head wsel', 4, 32, 32, 3, [_s(64)], wsel=3, options=[]),
    _case('head y_group', 4, 32, 32, 3, [_s(64)], y_group=2, options=[]),
    _case('head wsel y_group', 6, 32, 32, 8, [_s(96)], wsel=2, y_group=3, options=[]),
]


def _seg2mc(c):
    c['segs'].append(dict(SEG_DEFAULTS, C=16, ksize=1, ups=1, code=1, cmap=1))
    return c


OPTIONS['seg2mc'] = _seg2mc
OPTIONS['ycmap'] = _top(ycmap=1, Cy=96)
SWEEP = [o for o in OPTIONS if o not in ('seg2mc', 'ycmap')]          # what every base case is swept over


def pairs():
    """Every (base or mode case, option) pair of the two tables: (case name, option name, full case or None)."""
    out = []
    for b in BASE_CASES:
        for o in SWEEP:
            out.append((b['name'], o, apply_option(b, o)))
    for m in MODE_CASES:
        base = {k: v for k, v in m.items() if k != 'options'}
        for o in SWEEP + m['options']:
            out.append((m['name'], o, apply_option(base, o)))
    return out
