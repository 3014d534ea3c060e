"""The MCGlow kernels of csrc/glow_ops.hip one at a time, at CIFAR-10 widths (12 / 24 / 48 channels, 6 / 12 / 24 after a
split, NHWC rows padded to a multiple of 8) and at the limits of the LU kernels (C up to 64), in fp32 and bf16.

Every reference is float64 on the CPU, computed from exactly the values the kernel read (bf16 inputs are rounded to bf16
first).  Tolerances are derived from the output dtype and the length of the accumulation:

- u = 2^-24 is the fp32 unit roundoff.  A correctly rounded fp32 operation has relative error <= u.  The device expf /
  logf are accurate to 1 ulp, and 1 ulp <= 2u relative.  A chain of n fp32 additions or fmas has error at most
  n * u * (sum of the magnitudes of its terms), the usual gamma_n bound.
- A bf16 output is an fp32 value v rounded once to 8 significant bits: |bf16(v) - ref| <= |v - ref| + 2^-8 * |v|.
- Where a bound is "doubled", the factor 2 covers second-order terms and the u-versus-ulp slack of the count.

Where a row has padding, destination buffers start as NaN.  Padded channels must come out exactly 0 where the op writes
them, and channels outside the op's target range must still be NaN afterwards.  Inputs carry NaN in every channel the
op must not read, so a read of one shows up as a NaN in the result."""
import types

import pytest
import torch

from mcgen_amd._lib import CONSTANTS

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U16 = 2.0 ** -8
NAN = float('nan')
CIFAR_WIDTHS = [(12, 16), (6, 8), (24, 24), (48, 48)]     # (logical channels, NHWC row pitch)
DTYPES = [torch.float32, torch.bfloat16]


def _ops():
    from mcgen_amd import ops
    return ops


def _lib():
    from mcgen_amd import _lib as L
    return L.load()


def _dt(dtype):
    return _ops()._dt(dtype)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ck(rc, what):
    from mcgen_amd._lib import check
    check(rc, what)


def _out_tol(ref, t32, dtype):
    """Bound for an output computed in fp32 to within t32 of ref, then stored in `dtype`."""
    return t32 if dtype == torch.float32 else t32 + U16 * (ref.abs() + t32)


def _assert_within(got, ref, tol, what):
    err = (got.detach().double().cpu() - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {err.numel()} outside the bound; first at flat index {i}: '
                             f'got {float(got.flatten()[i])}, ref {float(ref.flatten()[i])}, tol {float(tol.flatten()[i])}')


def _padded(shape_px, c, cp, dtype, gen, scale=1.0, shift=0.0):
    """An NHWC tensor [*shape_px, cp] with random logical channels [0, c) and NaN padding; returns (device tensor, fp64
    copy of the logical channels exactly as stored)."""
    v = (torch.randn(*shape_px, c, generator=gen) * scale + shift).to(dtype)
    t = torch.full((*shape_px, cp), NAN, dtype=dtype)
    t[..., :c] = v
    return t.cuda(), v.double()


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device='cuda')


# ---- 1. LU kernels (fp32) --------------------------------------------------------------------------------------------
def _lu_params(c, gen):
    """LU factors of the QR of a random matrix (as InvConv2dLU builds them), w_s moved by up to +-0.5, and random junk
    outside the strict triangles of w_l / w_u, which the kernels must mask out."""
    q, _ = torch.linalg.qr(torch.randn(c, c, generator=gen, dtype=torch.float64))
    p, lo, up = torch.linalg.lu(q)
    s = torch.diagonal(up)
    ws = torch.log(s.abs()) + torch.rand(c, generator=gen, dtype=torch.float64) - 0.5
    low = torch.tril(torch.ones(c, c, dtype=torch.bool), -1)
    wl = torch.where(low, lo, torch.randn(c, c, generator=gen, dtype=torch.float64))
    wu = torch.where(low.T, up, torch.randn(c, c, generator=gen, dtype=torch.float64))
    prm = {'w_p': p, 'w_l': wl, 'w_u': wu, 'w_s': ws, 's_sign': torch.sign(s)}
    return {k: v.float().contiguous() for k, v in prm.items()}


def _lu_state64(prm):
    c = prm['w_s'].numel()
    sd = {k: v.double() for k, v in prm.items()}
    sd['u_mask'] = torch.triu(torch.ones(c, c, dtype=torch.float64), 1)
    sd['l_mask'] = sd['u_mask'].T.contiguous()
    sd['l_eye'] = torch.eye(c, dtype=torch.float64)
    return sd


def _lu_factors64(sd):
    lm = sd['w_l'] * sd['l_mask'] + sd['l_eye']
    um = sd['w_u'] * sd['u_mask'] + torch.diag(sd['s_sign'] * torch.exp(sd['w_s']))
    return lm, um


def _w_tol(prm):
    """|W - W64| <= 2 (C + 2) u (P |L| |U|): L U is a chain of C fmas per entry, exp(w_s) adds 1 ulp to U's diagonal,
    and P A is exact because P is a permutation (fmas with 0 and 1); doubled."""
    sd = _lu_state64(prm)
    lm, um = _lu_factors64(sd)
    c = prm['w_s'].numel()
    return 2 * (c + 2) * U32 * (sd['w_p'].abs() @ lm.abs() @ um.abs())


@pytest.mark.parametrize('c', [1, 2, 3, 12, 24, 48, 53, 64])
def test_invconv_weight_and_inverse(c):
    """W against the fp64 invconv_lu_weight, elementwise to the bound of _w_tol.  W^-1 from the in-kernel Gauss-Jordan
    against the fp64 inverse of the fp64 W, normwise: ||X - W^-1||_F <= 8 C u cond_F(W) ||W^-1||_F.  Gauss-Jordan with
    partial pivoting has a backward error of order C u per column; the rounding of W itself (_w_tol) is of the same
    order and doubles it; the u-versus-ulp slack doubles it again: 8 = 2 * 2 * 2."""
    from oracle import mcglow_oracle as G
    gen = torch.Generator().manual_seed(100 + c)
    prm = _lu_params(c, gen)
    dev = {k: v.cuda() for k, v in prm.items()}
    w, winv = _ops().invconv_weight(dev['w_p'], dev['w_l'], dev['w_u'], dev['w_s'], dev['s_sign'], inverse=True)
    torch.cuda.synchronize()
    ref = G.invconv_lu_weight(_lu_state64(prm), '')
    _assert_within(w, ref, _w_tol(prm), f'W at C={c}')
    inv = torch.linalg.inv(ref)
    cond = float(torch.linalg.norm(ref) * torch.linalg.norm(inv))
    err = float(torch.linalg.norm(winv.double().cpu() - inv))
    bound = 8 * c * U32 * cond * float(torch.linalg.norm(inv))
    assert err <= bound, (c, err, bound, cond)
    w2, none = _ops().invconv_weight(dev['w_p'], dev['w_l'], dev['w_u'], dev['w_s'], dev['s_sign'], inverse=False)
    assert none is None and torch.equal(w2, w)


def _invconv_bwd_ref(prm, dw, ld_coef):
    """fp64 autograd of <W(w_l, w_u, w_s), dW> + ld_coef * sum(w_s) through invconv_lu_weight, and the magnitude
    matrices of the kernel's three products (A = P^T dW exactly; dL = A U^T; dU = L^T A)."""
    from oracle import mcglow_oracle as G
    sd = _lu_state64(prm)
    for k in ('w_l', 'w_u', 'w_s'):
        sd[k].requires_grad_(True)
    ((G.invconv_lu_weight(sd, '') * dw).sum() + ld_coef * sd['w_s'].sum()).backward()
    with torch.no_grad():
        lm, um = _lu_factors64(sd)
        a = sd['w_p'].T @ dw
        m_l, m_u = a.abs() @ um.abs().T, lm.abs().T @ a.abs()
        m_s = torch.diagonal(m_u) * torch.exp(sd['w_s'])
    return sd['w_l'].grad, sd['w_u'].grad, sd['w_s'].grad, m_l, m_u, m_s


@pytest.mark.parametrize('c', [1, 2, 3, 12, 24, 48, 53, 64])
@pytest.mark.parametrize('pad_ld', [0, 8])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_invconv_bwd(c, pad_ld, accumulate):
    """dw_l / dw_u / dw_s against fp64 autograd, with ld_coef != 0, dW rows of pitch ldw = C or C + 8 (the extra columns
    NaN: never read), and accumulate 0 / 1 (outputs preloaded with known values).  Each gradient entry is one C-term fma
    chain over exactly computed A = P^T dW: error <= C u (|A||U|^T) for dw_l, C u (|L|^T|A|) for dw_u; dw_s adds exp
    (1 ulp), one product and the + ld_coef (1 rounding each); accumulating adds one more rounding of the result.  Bound
    2 (C + 4) u * magnitude (+ 2u |result|).  Not accumulating, every entry outside the strict triangles is exactly 0;
    accumulating, it keeps its preloaded value bit for bit."""
    gen = torch.Generator().manual_seed(200 + c)
    prm = _lu_params(c, gen)
    dw = torch.randn(c, c, generator=gen, dtype=torch.float64).float()
    dwbuf = torch.full((c, c + pad_ld), NAN)
    dwbuf[:, :c] = dw
    ld_coef = -37.25
    gl, gu, gs, m_l, m_u, m_s = _invconv_bwd_ref(prm, dw.double(), ld_coef)
    pre = [torch.randn(c, c, generator=gen), torch.randn(c, c, generator=gen), torch.randn(c, generator=gen)]
    outs = [p.clone().cuda() if accumulate else torch.full(p.shape, NAN, device='cuda') for p in pre]
    dev = {k: v.cuda() for k, v in prm.items()}
    _ops().invconv_bwd(dev['w_p'], dev['w_l'], dev['w_u'], dev['w_s'], dev['s_sign'], dwbuf.cuda(), ld_coef,
                       *outs, accumulate=bool(accumulate))
    torch.cuda.synchronize()
    base = [p.double() if accumulate else torch.zeros_like(p, dtype=torch.float64) for p in pre]
    low = torch.tril(torch.ones(c, c, dtype=torch.bool), -1)
    for got, b, g, m, mask, name in ((outs[0], base[0], gl, m_l, low, 'dw_l'), (outs[1], base[1], gu, m_u, low.T, 'dw_u')):
        ref = b + g
        tol = 2 * (c + 4) * U32 * m + (2 * U32 * ref.abs() if accumulate else 0)
        _assert_within(got.cpu()[mask], ref[mask], tol[mask], f'{name} C={c}')
        outside = got.cpu()[~mask]
        if accumulate:
            assert torch.equal(outside, pre[0 if name == 'dw_l' else 1][~mask]), name
        else:
            assert torch.equal(outside, torch.zeros_like(outside)), name
    ref = base[2] + gs
    tol = 2 * (c + 4) * U32 * m_s + 2 * U32 * (gs.abs() + ref.abs())
    _assert_within(outs[2], ref, tol, f'dw_s C={c}')


def test_lu_kernels_refuse_c65():
    """C <= 64: C = 65 is refused with the op's message before any launch."""
    from mcgen_amd._lib import McgenError
    gen = torch.Generator().manual_seed(65)
    dev = {k: v.cuda() for k, v in _lu_params(65, gen).items()}
    with pytest.raises(McgenError, match=r'C must be in 1\.\.64'):
        _ops().invconv_weight(dev['w_p'], dev['w_l'], dev['w_u'], dev['w_s'], dev['s_sign'], inverse=True)
    outs = [torch.zeros(65, 65, device='cuda'), torch.zeros(65, 65, device='cuda'), torch.zeros(65, device='cuda')]
    with pytest.raises(McgenError, match='invconv_bwd: bad arguments'):
        _ops().invconv_bwd(dev['w_p'], dev['w_l'], dev['w_u'], dev['w_s'], dev['s_sign'], torch.zeros(65, 65, device='cuda'),
                           1.0, *outs)
    ic = types.SimpleNamespace(**dev)
    with pytest.raises(McgenError, match=r'C in 1\.\.64'):
        _ops().invconv_weight_batch([ic])


# ---- 2. batched forms equal the single forms -------------------------------------------------------------------------
# Both forms run one __device__ body per job, so each job of a batch must reproduce its single-form launch bit for bit.
def _n_jobs(cap):
    return 2 * cap + 5


def test_invconv_weight_batch_matches_single():
    """2 * MCGEN_GLOW_BATCH_MAX + 5 jobs of mixed C: three launches.  Each W equals the single form bit for bit and the
    fp64 W to the bound of _w_tol."""
    from oracle import mcglow_oracle as G
    gen = torch.Generator().manual_seed(7)
    cs = [12, 24, 48, 6, 3, 53, 64, 1]
    n = _n_jobs(CONSTANTS['MCGEN_GLOW_BATCH_MAX'])
    prms = [_lu_params(cs[i % len(cs)], gen) for i in range(n)]
    ics = [types.SimpleNamespace(**{k: v.cuda() for k, v in p.items()}) for p in prms]
    ws = _ops().invconv_weight_batch(ics)
    for i, (p, ic, w) in enumerate(zip(prms, ics, ws)):
        single, _ = _ops().invconv_weight(ic.w_p, ic.w_l, ic.w_u, ic.w_s, ic.s_sign)
        assert torch.equal(w, single), i
        _assert_within(w, G.invconv_lu_weight(_lu_state64(p), ''), _w_tol(p), f'job {i}')


def test_actnorm_affine_batch_matches_single():
    """2 * MCGEN_GLOW_BATCH_MAX + 5 ActNorms of mixed C / Cp.  a = scale and negloc = -loc are exact, b = scale * loc is
    one fp32 rounding, i.e. the fp32 product computed on the CPU; every padded entry is exactly 0, and the single form
    (into NaN-filled buffers) writes the same bits."""
    gen = torch.Generator().manual_seed(8)
    widths = CIFAR_WIDTHS + [(3, 8), (32, 32), (130, 136)]
    n = _n_jobs(CONSTANTS['MCGEN_GLOW_BATCH_MAX'])
    ans, cps = [], []
    for i in range(n):
        c, cp = widths[i % len(widths)]
        ans.append(types.SimpleNamespace(loc=torch.randn(1, c, 1, 1, generator=gen).cuda(),
                                         scale=(torch.rand(1, c, 1, 1, generator=gen) + 0.5).cuda()))
        cps.append(cp)
    got = _ops().actnorm_affine_batch(ans, cps)
    lib = _lib()
    for i, (an, cp, (a, b, nl)) in enumerate(zip(ans, cps, got)):
        c = an.loc.numel()
        loc, sc = an.loc.view(-1).cpu(), an.scale.view(-1).cpu()
        z = torch.zeros(cp - c)
        assert torch.equal(a.cpu(), torch.cat([sc, z])), i
        assert torch.equal(b.cpu(), torch.cat([sc * loc, z])), i
        assert torch.equal(nl.cpu(), torch.cat([-loc, z])), i
        s = _nan((3, cp), torch.float32)
        _ck(lib.mcgen_actnorm_affine(an.loc.data_ptr(), an.scale.data_ptr(), c, cp, s[0].data_ptr(), s[1].data_ptr(),
                                     s[2].data_ptr(), _stream()), 'actnorm_affine')
        assert torch.equal(s, torch.stack([a, b, nl])), i


def _pld_ref(items, logdet0):
    """fp64 logdet0 + sum hw * (sum log|scale| + sum w_s), and its bound.  Each log term is 1 ulp (2u relative to |log|);
    the terms go through one sum of at most T = total terms fp32 additions/fmas (per thread, then the block tree), so
    error <= (T + 2) u sum hw |term| + 2 u |result|, doubled."""
    tot, mag, terms = 0.0, 0.0, 0
    for scale, ws, hw in items:
        ls, w = torch.log(scale.double().cpu().abs()), ws.double().cpu()
        tot += hw * (float(ls.sum()) + float(w.sum()))
        mag += hw * (float(ls.abs().sum()) + float(w.abs().sum()))
        terms += scale.numel() + ws.numel()
    ref = logdet0.double() + tot
    return ref, 2 * ((terms + 2) * U32 * mag + 2 * U32 * ref.abs())


def test_glow_param_logdet_single_and_batch():
    """glow_param_logdet per flow, and glow_param_logdet_batch over MCGEN_GLOW_PLD_MAX + 6 flows (two launches) of
    CIFAR-like sizes, into a preloaded logdet: both against fp64 (_pld_ref).  The batch adds all flows as ONE sum per
    launch (include/mcgen_hip.h), a different order of additions from a loop of single launches, so they are compared
    through the reference, not bit for bit."""
    gen = torch.Generator().manual_seed(9)
    n = CONSTANTS['MCGEN_GLOW_PLD_MAX'] + 6
    cs = [12, 24, 48, 64, 3, 300]
    items = []
    for i in range(n):
        c = cs[i % len(cs)]
        items.append(((torch.rand(c, generator=gen) * 2 + 0.2).cuda(), (torch.randn(c, generator=gen) * 0.3).cuda(),
                      [256, 64, 16, 4][i % 4]))
    logdet0 = torch.randn(5, generator=gen) * 100
    ld = logdet0.cuda()
    _ops().glow_param_logdet_batch(items, ld)
    ref, tol = _pld_ref(items, logdet0)
    _assert_within(ld, ref, tol, 'glow_param_logdet_batch')
    for i, (scale, ws, hw) in enumerate(items[:12]):
        one = logdet0.cuda()
        _ops().glow_param_logdet(scale, ws, hw, one)
        ref, tol = _pld_ref([(scale, ws, hw)], logdet0)
        _assert_within(one, ref, tol, f'glow_param_logdet {i}')


def _an_bwd_ref(part, scale, ld_coef, input_side, pre):
    """actnorm_bwd in fp64: s1 / s2 summed over tiles (the kernel sums in double: exact to fp64 rounding), rounded to fp32
    (u), then gl = s1 or s1 * scale (u), gs = s2 / scale or s2, + ld_coef / scale (3 roundings); + preload (u).
    Bound 2 * 5u (|s1| |scale| + |s2| / |scale| + |s2| + |ld_coef / scale| + |result|)."""
    s1, s2, sc = part[:, 0].double().sum(0), part[:, 1].double().sum(0), scale.double()
    gl = s1 if input_side else s1 * sc
    gs = (s2 / sc if input_side else s2) + ld_coef / sc
    rl, rs = pre[0].double() + gl, pre[1].double() + gs
    mag_l = s1.abs() * (1 + sc.abs()) + rl.abs()
    mag_s = s2.abs() * (1 + 1 / sc.abs()) + abs(ld_coef) / sc.abs() + rs.abs()
    return rl, rs, 10 * U32 * mag_l, 10 * U32 * mag_s


def _an_bwd_job(gen, c, pitch, tiles):
    part = torch.full((tiles, 2, pitch), NAN)
    part[:, :, :c] = torch.randn(tiles, 2, c, generator=gen)
    return part, torch.rand(c, generator=gen) + 0.5


def _pcs_job(gen, pixels, c, pitch, dtype):
    a, b = torch.full((pixels, pitch), NAN), torch.full((pixels, pitch), NAN)
    a[:, :c], b[:, :c] = torch.randn(pixels, c, generator=gen), torch.randn(pixels, c, generator=gen)
    return a.to(dtype), b.to(dtype)


def _pcs_ref(a, b, c, alpha, pre):
    """out = pre + alpha * sum_p a b in fp64.  A stage-1 chain, the four-wave sum and the stage-2 tree together add at
    most `pixels` terms, so error <= (pixels + 2) u |alpha| sum |a b| + 2u |result|, doubled."""
    ab = a[:, :c].double() * b[:, :c].double()
    ref = pre.double() + alpha * ab.sum(0)
    return ref, 2 * ((a.shape[0] + 2) * U32 * abs(alpha) * ab.abs().sum(0) + 2 * U32 * ref.abs())


def test_glow_deferred_matches_single():
    """ops.GlowDeferred with 2 * MCGEN_GLOW_BATCH_MAX + 5 jobs of each kind (actnorm_bwd_batch, prod_colsum_batch,
    invconv_bwd_batch), mixed C, mixed input_side / accumulate, prod_colsum on both sides of its 1024-pixel block-count
    switch: every output equals its single-form launch bit for bit and the fp64 reference to the bounds of _an_bwd_ref,
    _pcs_ref and test_invconv_bwd."""
    ops = _ops()
    gen = torch.Generator().manual_seed(10)
    n = _n_jobs(CONSTANTS['MCGEN_GLOW_BATCH_MAX'])
    dfr = ops.GlowDeferred()
    an, pcs, icb = [], [], []
    an_w = [(12, 16, 37), (48, 56, 300), (130, 136, 5), (6, 8, 1), (24, 24, 64)]
    for i in range(n):
        c, pitch, tiles = an_w[i % len(an_w)]
        part, scale = _an_bwd_job(gen, c, pitch, tiles)
        side, acc, ld = i % 2, (i // 2) % 2, 0.0 if i % 3 == 0 else 3.5 * (i + 1)
        pre = (torch.randn(c, generator=gen), torch.randn(c, generator=gen))
        bat = [p.clone().cuda() if acc else _nan((c,), torch.float32) for p in pre]
        one = [p.clone().cuda() if acc else _nan((c,), torch.float32) for p in pre]
        dfr.actnorm_bwd(part.cuda(), scale.cuda(), ld, side, *bat, accumulate=bool(acc))
        an.append((part, scale, ld, side, acc, pre, bat, one))
    pcs_w = [(700, 12, 16), (5000, 48, 56), (700, 70, 72), (5000, 6, 8), (1023, 24, 24), (1024, 24, 32)]
    for i in range(n):
        px, c, pitch = pcs_w[i % len(pcs_w)]
        a, b = _pcs_job(gen, px, c, pitch, torch.float32)
        acc, alpha = i % 2, 0.5 + i
        pre = torch.randn(c, generator=gen)
        bat = torch.full((c + 3,), NAN, device='cuda')
        one = torch.full((c + 3,), NAN, device='cuda')
        if acc:
            bat[:c], one[:c] = pre.cuda(), pre.cuda()
        ad, bd = a.cuda(), b.cuda()
        dfr.prod_colsum(ad, bd, c, bat, alpha=alpha, accumulate=bool(acc))
        pcs.append((a, b, ad, bd, c, alpha, acc, pre, bat, one))
    cs = [12, 24, 48, 6, 53, 3]
    for i in range(n):
        c = cs[i % len(cs)]
        prm = _lu_params(c, gen)
        ic = types.SimpleNamespace(**{k: v.cuda() for k, v in prm.items()})
        ldw = c + (8 if i % 2 else 0)
        dwbuf = torch.full((c, ldw), NAN)
        dwbuf[:, :c] = torch.randn(c, c, generator=gen)
        acc, ld = (i // 2) % 2, -1.5 * i
        pre = [torch.randn(c, c, generator=gen), torch.randn(c, c, generator=gen), torch.randn(c, generator=gen)]
        bat = [p.clone().cuda() if acc else torch.full(p.shape, NAN, device='cuda') for p in pre]
        one = [p.clone().cuda() if acc else torch.full(p.shape, NAN, device='cuda') for p in pre]
        dwd = dwbuf.cuda()
        dfr.invconv_bwd(ic, dwd, ld, *bat, accumulate=bool(acc))
        icb.append((prm, ic, dwbuf, dwd, ld, acc, pre, bat, one))
    dfr.run()
    for i, (part, scale, ld, side, acc, pre, bat, one) in enumerate(an):
        ops.actnorm_bwd(part.cuda(), scale.cuda(), ld, bool(side), *one, accumulate=bool(acc))
        assert torch.equal(bat[0], one[0]) and torch.equal(bat[1], one[1]), ('actnorm_bwd', i)
        rl, rs, tl, ts = _an_bwd_ref(part[:, :, :scale.numel()], scale, ld, side,
                                     pre if acc else (torch.zeros_like(pre[0]), torch.zeros_like(pre[1])))
        _assert_within(bat[0], rl, tl, f'actnorm_bwd dloc {i}')
        _assert_within(bat[1], rs, ts, f'actnorm_bwd dscale {i}')
    for i, (a, b, ad, bd, c, alpha, acc, pre, bat, one) in enumerate(pcs):
        ops.prod_colsum(ad, bd, c, one[:c], alpha=alpha, accumulate=bool(acc))
        assert torch.equal(bat[:c], one[:c]), ('prod_colsum', i)
        assert torch.isnan(bat[c:]).all(), ('prod_colsum wrote past C', i)
        ref, tol = _pcs_ref(a, b, c, alpha, pre if acc else torch.zeros_like(pre))
        _assert_within(bat[:c], ref, tol, f'prod_colsum {i}')
    for i, (prm, ic, dwbuf, dwd, ld, acc, pre, bat, one) in enumerate(icb):
        ops.invconv_bwd(ic.w_p, ic.w_l, ic.w_u, ic.w_s, ic.s_sign, dwd, ld, *one, accumulate=bool(acc))
        for k in range(3):
            assert torch.equal(bat[k], one[k]), ('invconv_bwd', i, k)
        c = prm['w_s'].numel()
        gl, gu, gs, m_l, m_u, m_s = _invconv_bwd_ref(prm, dwbuf[:, :c].double(), ld)
        low = torch.tril(torch.ones(c, c, dtype=torch.bool), -1)
        base = [p.double() if acc else torch.zeros_like(p, dtype=torch.float64) for p in pre]
        for k, (g, m, mask) in enumerate(((gl, m_l, low), (gu, m_u, low.T))):
            ref = base[k] + g
            tol = 2 * (c + 4) * U32 * m + 2 * U32 * ref.abs()
            _assert_within(bat[k].cpu()[mask], ref[mask], tol[mask], f'invconv_bwd {i}/{k}')
        ref = base[2] + gs
        _assert_within(bat[2], ref, 2 * (c + 4) * U32 * m_s + 2 * U32 * (gs.abs() + ref.abs()), f'invconv_bwd dw_s {i}')


# ---- 3. elementwise and reduction kernels, fp32 and bf16 -------------------------------------------------------------
def _squeeze64(x):
    n, h, w, c = x.shape
    return x.reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, 4 * c)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c', [3, 6, 12])
def test_glow_squeeze_unsqueeze(dtype, c):
    """Squeeze of c channels (padded to 8) into 4c (padded to pad8(4c)) and back: pure copies, so exact.  Padded
    channels come out exactly 0 on both sides (unsqueeze zero-fills them in its launcher), though every destination
    starts as NaN and every source pad is NaN."""
    ops = _ops()
    gen = torch.Generator().manual_seed(20 + c)
    n, h, w = 3, 8, 6
    cpb, cps = ops.pad8(c), ops.pad8(4 * c)
    x, x64 = _padded((n, h, w), c, cpb, dtype, gen)
    y = _nan((n, h // 2, w // 2, cps), dtype)
    lib = _lib()
    _ck(lib.mcgen_glow_squeeze(x.data_ptr(), y.data_ptr(), _dt(dtype), n, h, w, c, cpb, cps, 0, _stream()), 'squeeze')
    ref = _squeeze64(x64)
    yc = y.double().cpu()
    assert torch.equal(yc[..., :4 * c], ref)
    assert torch.equal(yc[..., 4 * c:], torch.zeros_like(yc[..., 4 * c:]))
    ys = y.clone()
    ys[..., 4 * c:] = NAN
    back = _nan((n, h, w, cpb), dtype)
    _ck(lib.mcgen_glow_squeeze(ys.data_ptr(), back.data_ptr(), _dt(dtype), n, h, w, c, cpb, cps, 1, _stream()), 'unsqueeze')
    bc = back.double().cpu()
    assert torch.equal(bc[..., :c], x64)
    assert torch.equal(bc[..., c:], torch.zeros_like(bc[..., c:]))
    assert torch.equal(ops.glow_unsqueeze(ops.glow_squeeze(x, c), 4 * c).double().cpu()[..., :c], x64)


def _coupling_ref(x64, h64, c):
    half = c // 2
    s = torch.sigmoid(h64[..., :half] + 2)
    t = h64[..., half:c]
    return s, t


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c,cp', CIFAR_WIDTHS)
def test_glow_coupling(dtype, c, cp):
    """Affine coupling forward / reverse and the per-sample log-determinant.
    s = 1 / (1 + expf(-(h_a + 2))) is within 6u of sigmoid (expf 1 ulp, an add, a division).  Forward
    y_b = (x_b + t) * s: error <= 8u (|x_b| + |t|) s, doubled.  Reverse x_b = y_b / s - t: error <= 8u (|y_b| / s + |t|),
    doubled.  y_a = x_a is a copy: exact.  logdet = sum over HW * C/2 of log s: each term within 8u (1 + |log s|)
    (logf 1 ulp, and s's 6u relative error is 6u absolute in log s), summed in one chain of at most HW * C/2 additions:
    error <= sum of term errors + (HW C/2) u sum |log s|, doubled; accumulating adds 2u |result|."""
    gen = torch.Generator().manual_seed(30 + c)
    n, h, w = 3, 8, 8
    half = c // 2
    x, x64 = _padded((n, h, w), c, cp, dtype, gen)
    hh, h64 = _padded((n, h, w), c, cp, dtype, gen)
    s, t = _coupling_ref(x64, h64, c)
    lib = _lib()
    for accumulate in (0, 1):
        ld0 = torch.randn(n, generator=gen) * 10
        ld = ld0.cuda() if accumulate else _nan((n,), torch.float32)
        y = _nan((n, h, w, cp), dtype)
        _ck(lib.mcgen_glow_coupling(x.data_ptr(), hh.data_ptr(), y.data_ptr(), _dt(dtype), ld.data_ptr(), n, h * w, c, cp, 0,
                                    accumulate, _stream()), 'glow_coupling')
        yc = y.double().cpu()
        assert torch.equal(yc[..., :half], x64[..., :half])
        ref = (x64[..., half:] + t) * s
        _assert_within(yc[..., half:c], ref, _out_tol(ref, 16 * U32 * (x64[..., half:].abs() + t.abs()) * s, dtype),
                       f'coupling y_b {dtype} C={c}')
        assert torch.equal(yc[..., c:], torch.zeros_like(yc[..., c:])), 'padded channels of y'
        logs = torch.log(s).reshape(n, -1)
        lref = logs.sum(1) + (ld0.double() if accumulate else 0)
        m = half * h * w
        ltol = 2 * ((8 * U32 * (1 + logs.abs())).sum(1) + m * U32 * logs.abs().sum(1) + 2 * U32 * lref.abs())
        _assert_within(ld, lref, ltol, f'coupling logdet acc={accumulate}')
    yin, y64 = _padded((n, h, w), c, cp, dtype, gen)
    xb = _nan((n, h, w, cp), dtype)
    _ck(lib.mcgen_glow_coupling(yin.data_ptr(), hh.data_ptr(), xb.data_ptr(), _dt(dtype), None, n, h * w, c, cp, 1, 0,
                                _stream()), 'glow_coupling reverse')
    xc = xb.double().cpu()
    assert torch.equal(xc[..., :half], y64[..., :half])
    ref = y64[..., half:] / s - t
    _assert_within(xc[..., half:c], ref, _out_tol(ref, 16 * U32 * (y64[..., half:].abs() / s + t.abs()), dtype),
                   f'coupling reverse {dtype} C={c}')
    assert torch.equal(xc[..., c:], torch.zeros_like(xc[..., c:]))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c,cp', CIFAR_WIDTHS)
def test_glow_coupling_bwd(dtype, c, cp):
    """Coupling backward against fp64 autograd of y = [v_a, (v_b + t) s] with dL/dlogdet = g.  dv_a = dy_a is a copy
    (exact); dv_b = dh_b = dy_b s: 8u |dy_b| s.  dh_a = dy_b (v_b + t) s (1 - s) + g (1 - s): 1 - s has absolute error
    <= 7u and s relative 6u, and four more roundings: error <= 8u (|dy_b| (|v_b| + |t|) s + |g|) + 4u |dh_a|; doubled.
    Padded channels of dv and dh are written exactly 0."""
    gen = torch.Generator().manual_seed(40 + c)
    n, h, w = 3, 8, 8
    half = c // 2
    v, v64 = _padded((n, h, w), c, cp, dtype, gen)
    hh, h64 = _padded((n, h, w), c, cp, dtype, gen)
    dy, dy64 = _padded((n, h, w), c, cp, dtype, gen)
    g = -0.37
    vr, hr = v64.clone().requires_grad_(True), h64.clone().requires_grad_(True)
    s = torch.sigmoid(hr[..., :half] + 2)
    y = torch.cat([vr[..., :half], (vr[..., half:] + hr[..., half:]) * s], -1)
    ((y * dy64).sum() + g * torch.log(s).sum()).backward()
    dv, dh = _nan((n, h, w, cp), dtype), _nan((n, h, w, cp), dtype)
    _ck(_lib().mcgen_glow_coupling_bwd(v.data_ptr(), hh.data_ptr(), dy.data_ptr(), dv.data_ptr(), dh.data_ptr(), _dt(dtype),
                                       g, n * h * w, c, cp, _stream()), 'glow_coupling_bwd')
    dvc, dhc = dv.double().cpu(), dh.double().cpu()
    s64 = s.detach()
    dyb, vb, t = dy64[..., half:], v64[..., half:], h64[..., half:]
    assert torch.equal(dvc[..., :half], dy64[..., :half])
    tb = 16 * U32 * dyb.abs() * s64
    _assert_within(dvc[..., half:c], vr.grad[..., half:], _out_tol(vr.grad[..., half:], tb, dtype), 'dv_b')
    _assert_within(dhc[..., half:c], hr.grad[..., half:], _out_tol(hr.grad[..., half:], tb, dtype), 'dh_b')
    ra = hr.grad[..., :half]
    ta = 2 * (8 * U32 * (dyb.abs() * (vb.abs() + t.abs()) * s64 + abs(g)) + 4 * U32 * ra.abs())
    _assert_within(dhc[..., :half], ra, _out_tol(ra, ta, dtype), 'dh_a')
    for o in (dvc, dhc):
        assert torch.equal(o[..., c:], torch.zeros_like(o[..., c:]))


def _prior(gen, px, cz, cpp, dtype):
    """prior rows [mean | log_sd] (2 cz channels) padded with NaN to cpp."""
    p = torch.full((*px, cpp), NAN)
    p[..., :cz] = torch.randn(*px, cz, generator=gen)
    p[..., cz:2 * cz] = torch.randn(*px, cz, generator=gen) * 0.5
    p = p.to(dtype)
    return p.cuda(), p[..., :cz].double(), p[..., cz:2 * cz].double()


def _z_rows(gen, px, cpz, c0, cz, dtype):
    """rows of cpz channels with z in [c0, c0 + cz), NaN elsewhere."""
    z = torch.full((*px, cpz), NAN)
    z[..., c0:c0 + cz] = torch.randn(*px, cz, generator=gen)
    z = z.to(dtype)
    return z.cuda(), z[..., c0:c0 + cz].double()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c,cp', CIFAR_WIDTHS)
def test_gaussian_logp_and_bwd(dtype, c, cp):
    """Prior log-density of the channels [c0, c0 + Cz) of z, c0 = Cz = C/2 (a split), prior rows padded with NaN; and its
    backward into dz at d0 != 0 with accumulate_dz.
    logp: each term -log sqrt(2 pi) - lsd - q, q = 0.5 d^2 e^(-2 lsd), within 8u (0.92 + |lsd| + q) (expf 1 ulp, five
    roundings); summed per sample over HW Cz terms: + (HW Cz) u sum |term|; accumulating + 2u |result|; doubled.
    backward: gz = -g d e: 6u |gz|; dmean = -gz exactly; dlsd = g (-1 + d^2 e): 8u |g| (1 + d^2 e); dz accumulated: + u of
    the result; doubled, then one bf16 rounding for bf16 outputs."""
    gen = torch.Generator().manual_seed(50 + c)
    n, h, w = 3, 8, 8
    cz = c // 2
    px = (n, h, w)
    z, z64 = _z_rows(gen, px, cp, cz, cz, dtype)
    prior, mean, lsd = _prior(gen, px, cz, ((2 * cz + 7) // 8 + 1) * 8, dtype)
    d = z64 - mean
    e = torch.exp(-2 * lsd)
    terms = (-0.9189385332046727 - lsd - 0.5 * d * d * e).reshape(n, -1)
    mag = (0.92 + lsd.abs() + 0.5 * d * d * e).reshape(n, -1)
    lp0 = torch.randn(n, generator=gen) * 50
    lp = lp0.cuda()
    _ops().gaussian_logp(z, cz, prior, cz, lp, accumulate=True)
    ref = lp0.double() + terms.sum(1)
    tol = 2 * ((8 * U32 * mag).sum(1) + terms.shape[1] * U32 * terms.abs().sum(1) + 2 * U32 * ref.abs())
    _assert_within(lp, ref, tol, f'gaussian_logp {dtype} C={c}')
    lp = _nan((n,), torch.float32)
    _ops().gaussian_logp(z, cz, prior, cz, lp, accumulate=False)
    _assert_within(lp, terms.sum(1), tol, 'gaussian_logp overwrite')
    # backward: dz rows of cp + 8 channels, target [d0, d0 + cz) preloaded, the rest NaN and untouched
    g, d0 = 0.61, 5
    dz = torch.full((*px, cp + 8), NAN)
    dz[..., d0:d0 + cz] = torch.randn(*px, cz, generator=gen)
    dz = dz.to(dtype)
    pre = dz[..., d0:d0 + cz].double()
    dzd = dz.cuda()
    dprior = _ops().gaussian_logp_bwd(z, cz, prior, cz, dzd, d0, g, True)
    gz = -g * d * e
    dzc, dpc = dzd.double().cpu(), dprior.double().cpu()
    rz = pre + gz
    _assert_within(dzc[..., d0:d0 + cz], rz, _out_tol(rz, 2 * (6 * U32 * gz.abs() + U32 * rz.abs()), dtype), 'dz')
    assert torch.isnan(dzc[..., :d0]).all() and torch.isnan(dzc[..., d0 + cz:]).all(), 'dz outside [d0, d0 + Cz) touched'
    _assert_within(dpc[..., :cz], -gz, _out_tol(gz, 12 * U32 * gz.abs(), dtype), 'dmean')
    rl = g * (-1 + d * d * e)
    _assert_within(dpc[..., cz:2 * cz], rl, _out_tol(rl, 16 * U32 * abs(g) * (1 + d * d * e), dtype), 'dlog_sd')
    assert torch.equal(dpc[..., 2 * cz:], torch.zeros_like(dpc[..., 2 * cz:])), 'dprior padding'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c,cp', CIFAR_WIDTHS)
def test_gaussian_sample_and_copy_channels(dtype, c, cp):
    """gaussian_sample into the channels [C/2, C) of a NaN-filled row (out = mean + expf(lsd) eps: 2 * (2u + 2u) of
    |mean| + e^lsd |eps|, then one bf16 rounding), and copy_channels from s0 != 0 to c0 != 0 (exact).  Channels outside the
    target range are still NaN afterwards; the sources carry NaN in every channel the ops must not read."""
    gen = torch.Generator().manual_seed(60 + c)
    n, h, w = 3, 8, 8
    px = (n, h, w)
    cz = c // 2
    eps, eps64 = _padded(px, cz, cp, dtype, gen)
    prior, mean, lsd = _prior(gen, px, cz, ((2 * cz + 7) // 8 + 1) * 8, dtype)
    out = _nan((*px, cp), dtype)
    _ops().gaussian_sample(eps, prior, out, cz, cz)
    oc = out.double().cpu()
    ref = mean + torch.exp(lsd) * eps64
    _assert_within(oc[..., cz:c], ref, _out_tol(ref, 8 * U32 * (mean.abs() + torch.exp(lsd) * eps64.abs()), dtype),
                   f'gaussian_sample {dtype} C={c}')
    assert torch.isnan(oc[..., :cz]).all() and torch.isnan(oc[..., c:]).all()
    s0, c0, cn = 2, 3, c - 2
    src = torch.full((*px, c + 2), NAN)
    src[..., s0:s0 + cn] = torch.randn(*px, cn, generator=gen)
    src = src.to(dtype)
    dst = _nan((*px, cp + 8), dtype)
    _ops().copy_channels(src.cuda(), s0, dst, c0, cn)
    dc = dst.cpu()
    assert torch.equal(dc[..., c0:c0 + cn], src[..., s0:s0 + cn])
    assert torch.isnan(dc[..., :c0]).all() and torch.isnan(dc[..., c0 + cn:]).all()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c,cp', CIFAR_WIDTHS)
def test_channel_stats_actnorm_init(dtype, c, cp):
    """ActNorm's data-dependent init from channel_stats partials: loc = -mean, scale = 1 / (unbiased std + 1e-6), with
    pixel counts that the block count does not divide (189 pixels over 64 blocks leaves the last block empty; over 10
    blocks, the last one short).  Pads of x are NaN: the init must not read their partials.
    Per block, s1 and s2 are fp32 chains of ppb = ceil(pixels / blocks) terms (s2 of fmas); the blocks are added in
    double.  |ds1| <= ppb u sum|x|, |ds2| <= (ppb + 1) u sum x^2.  loc: |ds1| / count + u |mean|.  var = (s2 - s1 mean) /
    (count - 1) moves by (|ds2| + 2 |mean| |ds1|) / (count - 1), std by that over 2 std, and scale by 1 / (std + 1e-6)^2
    times that, plus 3u for its own roundings; doubled."""
    ops = _ops()
    gen = torch.Generator().manual_seed(70 + c)
    n, h, w = 3, 7, 9
    x, x64 = _padded((n, h, w), c, cp, dtype, gen, scale=3.0, shift=1.0)
    flat = x64.reshape(-1, c)
    count = flat.shape[0]
    mean, std = flat.mean(0), flat.std(0)
    for blocks in (64, 10):
        part = ops.channel_stats(x, blocks=blocks)
        loc, scale = _nan((1, c, 1, 1), torch.float32), _nan((1, c, 1, 1), torch.float32)
        ops.actnorm_init(part, count, loc, scale)
        ppb = -(-count // part.shape[0])
        ds1 = ppb * U32 * flat.abs().sum(0)
        ds2 = (ppb + 1) * U32 * (flat * flat).sum(0)
        _assert_within(loc.view(-1), -mean, 2 * (ds1 / count + U32 * mean.abs()), f'loc blocks={blocks}')
        dstd = (ds2 + 2 * mean.abs() * ds1) / (count - 1) / (2 * std)
        ref = 1 / (std + 1e-6)
        _assert_within(scale.view(-1), ref, 2 * (dstd * ref * ref + 3 * U32 * ref), f'scale blocks={blocks}')


@pytest.mark.parametrize('c,pitch,tiles', [(12, 16, 37), (48, 56, 300), (130, 136, 20)])
@pytest.mark.parametrize('input_side', [0, 1])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_actnorm_bwd(c, pitch, tiles, input_side, accumulate):
    """ActNorm parameter gradients from dgrad-epilogue partials (pads NaN, never read), ld_coef != 0, both input_side
    conventions, accumulate 0 / 1: against fp64 to the bound of _an_bwd_ref.  C = 130 takes three blocks."""
    gen = torch.Generator().manual_seed(80 + c)
    part, scale = _an_bwd_job(gen, c, pitch, tiles)
    pre = (torch.randn(c, generator=gen), torch.randn(c, generator=gen))
    dloc = pre[0].cuda() if accumulate else _nan((c,), torch.float32)
    dscale = pre[1].cuda() if accumulate else _nan((c,), torch.float32)
    ld = 123.5
    _ops().actnorm_bwd(part.cuda(), scale.cuda(), ld, bool(input_side), dloc, dscale, accumulate=bool(accumulate))
    base = pre if accumulate else (torch.zeros(c), torch.zeros(c))
    rl, rs, tl, ts = _an_bwd_ref(part[:, :, :c], scale, ld, input_side, base)
    _assert_within(dloc, rl, tl, 'dloc')
    _assert_within(dscale, rs, ts, 'dscale')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('pixels', [700, 5000])
@pytest.mark.parametrize('c,pitch', [(12, 16), (48, 56), (70, 72)])
def test_prod_colsum(dtype, pixels, c, pitch):
    """out[c] (+)= alpha sum_p a b over rows of pitch > C (pads NaN, never read), on both sides of the 1024-pixel
    block-count switch, and C = 70 past one wave of channels; against fp64 to the bound of _pcs_ref.  Entries of out past
    C stay NaN."""
    gen = torch.Generator().manual_seed(90 + c)
    a, b = _pcs_job(gen, pixels, c, pitch, dtype)
    for accumulate in (0, 1):
        pre = torch.randn(c, generator=gen)
        out = torch.full((c + 4,), NAN, device='cuda')
        if accumulate:
            out[:c] = pre.cuda()
        _ops().prod_colsum(a.cuda(), b.cuda(), c, out[:c], alpha=-2.5, accumulate=bool(accumulate))
        ref, tol = _pcs_ref(a, b, c, -2.5, pre if accumulate else torch.zeros(c))
        _assert_within(out[:c], ref, tol, f'prod_colsum acc={accumulate}')
        assert torch.isnan(out[c:]).all()


@pytest.mark.parametrize('scale', [1.0, 1e-4])
def test_clip_grad_norm_large(scale):
    """clip_grad_norm_ on 3 000 001 elements: past 7 * 256 * 256, so the eight-loads-in-flight loop runs.  Each thread's
    fp32 chain has L = ceil(n / 65536) = 46 fmas, the block sum 6 shuffles plus 4 waves, the 256 block sums are added
    in double: the squared norm is within (L + 11) u relative, the norm within half that plus u for its rounding.
    Above max_norm (norm ~ 1732) every element is scaled by max_norm / (norm + 1e-6): the ratio adds 2u, the product u,
    doubled.  Below it (norm ~ 0.17) nothing changes, bit for bit."""
    gen = torch.Generator().manual_seed(12)
    n = 3_000_001
    g = torch.randn(n, generator=gen) * scale
    gd = g.cuda()
    nrm = float(_ops().clip_grad_norm_(gd, 1.0))
    ref = float(torch.linalg.norm(g.double()))
    rel = ((-(-n // 65536) + 11) / 2 + 1) * U32
    assert abs(nrm - ref) <= rel * ref, (nrm, ref, rel * ref)
    if ref > 1.0:
        want = g.double() / (ref + 1e-6)
        _assert_within(gd, want, 2 * (rel + 3 * U32) * want.abs(), 'clipped gradient')
    else:
        assert torch.equal(gd.cpu(), g)
