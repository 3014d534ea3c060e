"""The kernels of csrc/pixelcnn_ops.hip and csrc/vq_ops.hip one at a time (MCPixelCNN, CPixelCNN, MCVAE, CVAE, VQ-VAE and
the classifier use them), in fp32 and bf16, at the smallest shapes that reach each path: every tap geometry of the
engines on rectangular maps, every lane split of the two statistics kernels, blocks that straddle images, ragged and
empty blocks, the second trip of the grid-stride loops, the tail wave of vq_stats, both clamps of the BCE, ties and
non-finite rows of the arg-min.

Every reference is float64 on the CPU (tests/pixel_ops_ref.py, itself checked against torch in
test_pixel_ops_ref_cpu.py), computed from exactly the values the kernel read: bf16 inputs are rounded to bf16 first, fp32
scalars are passed as their fp32 value.  Tolerances are derived, not observed:

- u = 2^-24 is the fp32 unit roundoff.  A correctly rounded fp32 operation (+, *, fma) has relative error <= u; device
  division is counted as 1 ulp <= 2u, expf / logf as 1 ulp <= 2u.  A chain of n fp32 additions, in any order, has error at
  most n * u * (sum of the magnitudes of its terms).  fp64 accumulation has the same bound with 2^-53.
- A bf16 output is an fp32 value v rounded once: |bf16(v) - ref| <= |v - ref| + 2^-8 |v| (_out_tol).
- The accuracy of the device tanhf and log1pf is not documented in the project.  Both are ASSUMED accurate to 2 ulp
  (TANH_ULP, LOG1P_ULP).  test_device_tanhf_and_sigmoid_accuracy measures tanhf, and the sigmoid 1 / (1 + expf(-a))
  against its derived 5u, where each stands alone in an fp32 output, over |x| <= 20, prints the figures and fails if
  one exceeds what the bounds below assume.  Measured on an MI355X (ROCm 7.2): tanhf 1.297 ulp, the sigmoid 2.395 ulp.
- sigmoid: q = 1 / (1 + expf(-b)) has expf within 2u, the sum within u (the error of expf enters scaled by e / (1 + e)
  < 1) and the division within 2u: |dq| <= 5u q.
- Where a bound is "doubled", the factor 2 covers second-order terms and the u-versus-ulp slack of the count.
- Copies, masks and integer indices are bit-exact: plain im2col, q, counts, g_gated, argmin.

Destination buffers and row padding start as NaN; padded outputs the op writes must be exactly 0.  Inputs carry NaN in
every channel or buffer the op must not read."""
import math

import pytest
import torch

import pixel_ops_ref as R
from mcgen_amd._lib import CONSTANTS

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U16 = 2.0 ** -8
U64 = 2.0 ** -53
TINY = 2.0 ** -126          # smallest normal fp32: below it results lose bits or flush (expf overflows past 88.7)
NAN = float('nan')
INF = float('inf')
DTYPES = [torch.float32, torch.bfloat16]
TANH_ULP = 2                # assumed, see the module docstring
LOG1P_ULP = 2               # assumed, see the module docstring
GATED_MAX = CONSTANTS['MCGEN_GATED_MAX']
# thresholds that live only in the kernel sources and the wrappers
GRID_ITEMS = 4096 * 256     # grid_for: 4096 blocks of 256 threads; the grid-stride loops take a second trip above this
VQ_PC = 128                 # vq_ops.hip: pixels per statistics chunk
VQ_KT = 64                  # vq_ops.hip: codes per workgroup
VQ_DMAX = 64                # vq_ops.hip: largest embedding size (four waves of 16 features)
RED_SLOTS = 64              # small_ops.hip reduce_partials: row slots per block
LOSS_BLOCKS = 1024          # ops.bce_logits / ops.mse_tanh: blocks at most
# geometries (kh, kw, oh, ow, stride) of the engines: mask-A 7x7 as 4x7 + 1x4, mask-B 3x3 as 2x3 + 1x2, MCVAE's stride 2
GEOMS = [(4, 7, 3, 3, 1), (1, 4, 0, 3, 1), (2, 3, 1, 1, 1), (1, 2, 0, 1, 1), (4, 4, 1, 1, 2)]


def _stats_blocks(pixels):
    """ops.gated_bwd / ops.code_bn_bwd: one block per 16 pixels, 256 at most."""
    return max(1, min(256, pixels // 16))


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


def _p(t):
    return None if t is None else t.data_ptr()


def _out_tol(ref, t32, dtype):
    """Bound for an output computed in fp32 to within t32 of ref, then stored in `dtype`."""
    return t32 if dtype == torch.float32 else t32 + U16 * (ref.abs() + t32)


def _assert_within(got, ref, tol, what):
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        tol = tol.expand_as(ref) if torch.is_tensor(tol) else torch.full_like(ref, tol)
        raise AssertionError(f'{what}: {int(bad.sum())} of {err.numel()} outside the bound; first at flat index {i}: '
                             f'got {float(got.flatten()[i])}, ref {float(ref.flatten()[i])}, tol {float(tol.flatten()[i])}')


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _assert_bits(got, ref, what):
    assert got.dtype == ref.dtype and torch.equal(_bits(got).reshape(-1), _bits(ref).reshape(-1)), what


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device='cuda')


def _randn(gen, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=gen).to(dtype)


def _vec(gen, c, scale=1.0, shift=0.0):
    return torch.randn(c, generator=gen) * scale + shift


# ---- 0. the two device functions whose accuracy the bounds assume ------------------------------------------------------
def _ulps(got, ref):
    """|got - ref| in units of the fp32 ulp at ref."""
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(TINY))) - 23)
    return float(((got.double() - ref).abs() / ulp).max())


def test_device_tanhf_and_sigmoid_accuracy(capsys):
    """The fp32 `decoded` of mse_tanh is tanhf(x) and nothing else; the fp32 `recon` of bce_logits is 1 / (1 + expf(-a)).
    400 001 points over |x| <= 20 (step 1e-4) and 20 000 points over |x| <= 1e-2.  tanhf must be within TANH_ULP ulp,
    the sigmoid within 5u, i.e. 5 ulp at most (an ulp is at least u relative)."""
    x = torch.cat([torch.linspace(-20, 20, 400001), torch.linspace(-1e-2, 1e-2, 20000)])
    n = (x.numel() + 7) // 8 * 8
    xp = torch.zeros(n)
    xp[:x.numel()] = x
    xd = xp.view(-1, 8).cuda()
    dec, _, _ = _ops().mse_tanh(xd, torch.zeros_like(xd), 8, 1.0, False)
    rec, _, _ = _ops().bce_logits(xd, torch.zeros_like(xd), 8, 1.0, False)
    torch.cuda.synchronize()
    t_ulp = _ulps(dec.cpu().view(-1), torch.tanh(xp.double()))
    s_ulp = _ulps(rec.cpu().view(-1), torch.sigmoid(xp.double()))
    with capsys.disabled():
        print(f'\n[measured] device tanhf: {t_ulp:.3f} ulp (assumed {TANH_ULP}); 1 / (1 + expf(-a)): {s_ulp:.3f} ulp (derived 5)')
    assert t_ulp <= TANH_ULP and s_ulp <= 5, (t_ulp, s_ulp)


# ---- 1. im2col / col2im ---------------------------------------------------------------------------------------------
def _im2col(x, geom, scale=None, shift=None, relu=False, code=None):
    """mcgen_im2col into a NaN-filled destination."""
    kh, kw, oh, ow, stride = geom
    n, h, w, cp = x.shape
    col = _nan((n, h // stride, w // stride, kh * kw * cp), x.dtype)
    _ck(_lib().mcgen_im2col(_p(x), _p(col), _dt(x.dtype), n, h, w, cp, kh, kw, oh, ow, stride, _p(scale), _p(shift), int(relu),
                            _p(code), _stream()), 'im2col')
    torch.cuda.synchronize()
    return col


def _prologue_tol(ref, dtype):
    """z = fma(x, scale, shift) is one rounding and keeps the sign of the exact z, relu is exact, * code is one more:
    |d out| <= 2u |out|; doubled."""
    return _out_tol(ref, 4 * U32 * ref.abs(), dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS)
def test_im2col(geom, dtype):
    """N = 3, 6 x 10 maps, Cp = 8 / 24 / 128.  Plain im2col is a copy: bit-exact, zeros outside the map.  With a prologue
    (affine only, relu only, code only, all three; codes are real-valued with both signs, so relu(z) * code differs from
    relu(z * code)) the bound is _prologue_tol and every out-of-map tap is still exactly 0."""
    kh, kw, oh, ow, stride = geom
    for cp in (8, 24, 128):
        gen = torch.Generator().manual_seed(cp + kh * kw)
        x = _randn(gen, 3, 6, 10, cp, dtype=dtype)
        sc, sh, code = _vec(gen, cp), _vec(gen, cp, 0.5), torch.randn(3, cp, generator=gen)
        assert (code < 0).any()
        xd = x.cuda()
        plain = R.im2col(x, kh, kw, oh, ow, stride)
        _assert_bits(_im2col(xd, geom), plain.to(dtype), f'plain {geom} Cp={cp}')
        _assert_bits(_ops().im2col(xd, kh, kw, oh, ow, stride), plain.to(dtype), f'wrapper {geom} Cp={cp}')
        outside = R.im2col(torch.ones_like(x), kh, kw, oh, ow, stride) == 0
        assert outside.any() or (kh, kw) == (1, 1)
        for a, r, k in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            kw_ref = dict(scale=sc if a else None, shift=sh if a else None, relu=bool(r), code=code if k else None)
            got = _im2col(xd, geom, sc.cuda() if a else None, sh.cuda() if a else None, bool(r), code.cuda() if k else None)
            ref = R.im2col(x, kh, kw, oh, ow, stride, **kw_ref)
            _assert_within(got, ref, _prologue_tol(ref, dtype), f'prologue {(a, r, k)} {geom} Cp={cp}')
            assert bool((got.cpu()[outside] == 0).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_im2col_past_the_grid_cap(dtype):
    """2 x 300 x 292 at Cp = 8 with 2 x 3 taps: 1 051 200 vectors of 8, the grid's 1 048 576 and a ragged 2 624 more.  The
    full prologue with one code per image, so a wrong pixel or image index in the second trip changes values."""
    geom = (2, 3, 1, 1, 1)
    gen = torch.Generator().manual_seed(1)
    x = _randn(gen, 2, 300, 292, 8, dtype=dtype)
    assert GRID_ITEMS < x.numel() // 8 * 6 < GRID_ITEMS + 4096 and (x.numel() // 8 * 6) % 256
    sc, sh, code = _vec(gen, 8), _vec(gen, 8, 0.5), torch.randn(2, 8, generator=gen)
    _assert_bits(_im2col(x.cuda(), geom), R.im2col(x, *geom).to(dtype), 'plain')
    got = _im2col(x.cuda(), geom, sc.cuda(), sh.cuda(), True, code.cuda())
    ref = R.im2col(x, *geom, scale=sc, shift=sh, relu=True, code=code)
    _assert_within(got, ref, _prologue_tol(ref, dtype), 'prologue')


def _col2im(dcol, shape, geom, bias=None, c=0, base=None):
    """mcgen_col2im into a NaN-filled dx, or accumulating onto `base`."""
    kh, kw, oh, ow, stride = geom
    n, h, w, cp = shape
    dx = _nan(shape, dcol.dtype) if base is None else base.clone()
    _ck(_lib().mcgen_col2im(_p(dcol), _p(dx), _dt(dcol.dtype), n, h, w, cp, kh, kw, oh, ow, stride, _p(bias), c,
                            int(base is not None), _stream()), 'col2im')
    torch.cuda.synchronize()
    return dx


def _col2im_tol(dcol, cp, geom, dtype, bias=None, base=None):
    """dx starts from bias (or the loaded dx) and adds at most kh * kw taps in fp32: a chain of kh * kw additions over
    |start| + sum |dcol|, doubled."""
    kh, kw, oh, ow, stride = geom
    mag = R.col2im(dcol.double().abs(), cp, kh, kw, oh, ow, stride, None if bias is None else bias.abs(),
                   None if base is None else base.double().abs())
    ref = R.col2im(dcol, cp, kh, kw, oh, ow, stride, bias, base)
    return ref, _out_tol(ref, 2 * kh * kw * U32 * mag, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('geom', GEOMS)
def test_col2im(geom, dtype):
    """Elementwise against the fp64 adjoint on 3 x 6 x 10 maps, Cp = 8 / 24 / 128: without bias, with a bias on C = Cp - 5
    channels (3 of 8: the other channels get none), and accumulating onto a non-zero dx (the bias is then ignored, as the
    engines rely on).  The wrapper gives the same bits."""
    kh, kw, oh, ow, stride = geom
    for cp in (8, 24, 128):
        gen = torch.Generator().manual_seed(cp + kh * kw + 1)
        shape = (3, 6, 10, cp)
        dcol = _randn(gen, 3, 6 // stride, 10 // stride, kh * kw * cp, dtype=dtype)
        bias = _vec(gen, cp - 5, 1.0, 3.0)
        base = _randn(gen, *shape, dtype=dtype)
        for b, a in ((None, None), (bias, None), (bias, base)):
            got = _col2im(dcol.cuda(), shape, geom, None if b is None else b.cuda(), 0 if b is None else b.numel(),
                          None if a is None else a.cuda())
            ref, tol = _col2im_tol(dcol, cp, geom, dtype, None if a is not None else b, a)
            _assert_within(got, ref, tol, f'col2im {geom} Cp={cp} bias={b is not None} accumulate={a is not None}')
        wr = _ops().col2im(dcol.cuda(), cp, kh, kw, oh, ow, stride, bias=bias.cuda())
        _assert_bits(wr, _col2im(dcol.cuda(), shape, geom, bias.cuda(), bias.numel()), 'wrapper')


@pytest.mark.parametrize('dtype', DTYPES)
def test_col2im_past_the_grid_cap(dtype):
    """2 x 724 x 725 at Cp = 8 with 1 x 2 taps: 1 049 800 vectors of 8, the grid's 1 048 576 and a ragged 1 224 more."""
    geom = (1, 2, 0, 1, 1)
    gen = torch.Generator().manual_seed(2)
    shape = (2, 724, 725, 8)
    assert GRID_ITEMS < 2 * 724 * 725 < GRID_ITEMS + 4096 and (2 * 724 * 725) % 256
    dcol = _randn(gen, 2, 724, 725, 16, dtype=dtype)
    bias = _vec(gen, 3, 1.0, 3.0)
    got = _col2im(dcol.cuda(), shape, geom, bias.cuda(), 3)
    ref, tol = _col2im_tol(dcol, 8, geom, dtype, bias)
    _assert_within(got, ref, tol, 'col2im')


# ---- 2. gated activation, forward ---------------------------------------------------------------------------------------
def _gated_case(n, hw, c, dtype, gen):
    s = _randn(gen, n, hw, 2 * c, dtype=dtype)
    s[..., c:] *= 3                                                         # sigmoid over its whole range
    sc, sh = _vec(gen, c), _vec(gen, c, 0.5)
    sc[0], sh[0] = 2.0, -1.0
    s[:, ::3, 0] = 0.5                                                      # z = 0 exactly: the ReLU's gradient there is 0
    return s, sc, sh, torch.randn(n, c, generator=gen)


def _gated_fwd(s, sc, sh, code):
    n, hw, c2 = s.shape
    out = _nan((n, hw, c2 // 2), s.dtype)
    _ck(_lib().mcgen_gated_fwd(_p(s), _p(sc), _p(sh), _p(code), _p(out), _dt(s.dtype), n, hw, c2 // 2, _stream()), 'gated_fwd')
    torch.cuda.synchronize()
    return out


def _gated_fwd_tol(ref, dtype):
    """out = (code * relu(z)) / (1 + expf(-b)): z one rounding (u), the product u, the denominator 3u (expf 2u scaled by
    e / (1 + e), the sum u), the division 2u: 7u |out|, doubled."""
    return _out_tol(ref, 14 * U32 * ref.abs(), dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c', [8, 64, 128])
def test_gated_fwd(c, dtype):
    gen = torch.Generator().manual_seed(c)
    s, sc, sh, code = _gated_case(3, 35, c, dtype, gen)
    got = _gated_fwd(s.cuda(), sc.cuda(), sh.cuda(), code.cuda())
    ref = R.gated_fwd(s, sc, sh, code)
    _assert_within(got, ref, _gated_fwd_tol(ref, dtype), f'gated_fwd C={c}')
    _assert_bits(_ops().gated_fwd(s.cuda().view(3, 5, 7, 2 * c), sc.cuda(), sh.cuda(), code.cuda()), got, 'wrapper')


@pytest.mark.parametrize('dtype', DTYPES)
def test_gated_fwd_batch_matches_single(dtype):
    """1 .. MCGEN_GATED_MAX jobs of unequal N, HW and C in one launch (the grid is sized by the largest, the others run
    out early): every job equals its single launch bit for bit."""
    gen = torch.Generator().manual_seed(3)
    dims = [(3, 35, 8), (1, 7, 64), (2, 16, 128), (5, 3, 16)]
    assert len(dims) == GATED_MAX
    cases = [[t.cuda() for t in _gated_case(n, hw, c, dtype, gen)] for n, hw, c in dims]
    singles = [_gated_fwd(*k) for k in cases]
    for n_jobs in range(1, GATED_MAX + 1):
        for order in (cases[:n_jobs], cases[::-1][:n_jobs]):
            outs = _ops().gated_fwd_batch([(s.view(s.shape[0], 1, s.shape[1], s.shape[2]), sc, sh, k) for s, sc, sh, k in order])
            torch.cuda.synchronize()
            for (s, *_), out in zip(order, outs):
                i = [id(k[0]) for k in cases].index(id(s))
                _assert_bits(out, singles[i], f'{n_jobs} jobs, job {i}')


@pytest.mark.parametrize('dtype', DTYPES)
def test_gated_fwd_past_the_grid_cap(dtype):
    """3 x 349 600 pixels at C = 8: 1 048 800 vectors, 224 past the grid."""
    gen = torch.Generator().manual_seed(4)
    assert GRID_ITEMS < 3 * 349600 < GRID_ITEMS + 4096 and (3 * 349600) % 256
    s, sc, sh, code = _gated_case(3, 349600, 8, dtype, gen)
    got = _gated_fwd(s.cuda(), sc.cuda(), sh.cuda(), code.cuda())
    ref = R.gated_fwd(s, sc, sh, code)
    _assert_within(got, ref, _gated_fwd_tol(ref, dtype), 'gated_fwd')


# ---- 3. the two statistics kernels and their apply passes ---------------------------------------------------------------
STATS_C = [8, 16, 64, 128, 256, 512, 2048]            # lanes = 256 / (C / 8) = 256, 128, 32, 16, 8, 4, 1
# (N, HW): 245 pixels in 15 blocks of 17 (blocks straddle the 49-pixel images, the last holds 7); 4112 pixels in 256 blocks
# of 17 (block 241 holds 15, blocks 242 .. 255 none)
STATS_PIXELS = [(5, 49), (257, 16)]
STATS_CASES = [(c, n, hw) for c in STATS_C for n, hw in STATS_PIXELS] + [(128, 8, 1024)]      # + the workload's 8192 pixels


def _check_partials(part, pixels, blocks, what):
    """Blocks past the last pixel wrote exactly 0 over the NaN; returns ppb."""
    ppb = (pixels + blocks - 1) // blocks
    first_empty = (pixels + ppb - 1) // ppb
    p = part.cpu()
    assert not torch.isnan(p).any(), f'{what}: a partial was not written'
    if first_empty < blocks:
        assert bool((p[first_empty:] == 0).all()), f'{what}: empty blocks must write 0'
    return ppb


def _sum_tol(term_ulps, terms_abs, s_ref, ppb, lanes, blocks):
    """A channel's sum: each term within term_ulps * u of its fp64 value; a lane adds ceil(ppb / lanes) terms, the block
    adds its lanes (fp32), mcgen_bn_bwd_finalize adds the blocks in fp64 and rounds once to fp32; doubled."""
    chain = (ppb + lanes - 1) // lanes + lanes
    return 2 * ((term_ulps + chain) * U32 * terms_abs + (blocks + RED_SLOTS) * U64 * terms_abs + U32 * s_ref.abs())


def _apply_tol(dz, x, sc, mean, rstd, s1, s2, inv, ref, dtype):
    """scale (dz - (s1 + xh s2) inv) or scale (dz - s1 inv - xh s2 inv), xh = (x - mean) rstd in fp32: with T1 = |dz|,
    T2 = |s1 inv|, T3 = |xh s2 inv| both forms are within |scale| (2u T1 + 5u T2 + 8u T3) + u |result|; doubled."""
    xh = (x.double() - mean.double()) * rstd.double()
    t1, t2, t3 = dz.double().abs(), (s1.double() * inv).abs(), (xh * s2.double() * inv).abs()
    t32 = 2 * (sc.double().abs() * (2 * U32 * t1 + 5 * U32 * t2 + 8 * U32 * t3) + U32 * ref.abs())
    return _out_tol(ref, t32, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c,n,hw', STATS_CASES)
def test_gated_bwd(c, n, hw, dtype):
    """mcgen_gated_bwd_stats, mcgen_bn_bwd_finalize and mcgen_gated_bwd_apply with the wrapper's block rule, each checked
    on its own; ops.gated_bwd then gives the same bits.
    Pass 1: dz = (g code) q [z > 0] is u + 5u + u = 7u |dz|; db = (g code) relu(z) q (1 - q) with A = |g code relu(z)|:
    the products 4u, q 5u, and 1 - q within 5u q + u (1 - q), so |d db| <= A q u (10 (1 - q) + 5 q) <= 10u A q; both
    doubled.  The sign of z is that of the exact z (one fma); where z = 0 exactly, dz = 0.  s1 = sum dz (terms within 7u), s2 = sum dz xhat (xhat 2u, the
    product u: 10u) by _sum_tol.  The sums use the unrounded dz.
    Pass 2 reads back the stored dz and the fp32 sums: its reference takes those very values, bound _apply_tol; the db half
    of ds keeps its bits."""
    ops, lib = _ops(), _lib()
    gen = torch.Generator().manual_seed(c + n)
    pixels = n * hw
    s, sc, sh, code = _gated_case(n, hw, c, dtype, gen)
    g = _randn(gen, n, hw, c, dtype=dtype)
    mean, rstd = _vec(gen, c, 0.5), torch.rand(c, generator=gen) + 0.5
    blocks = _stats_blocks(pixels)
    dev = [t.cuda() for t in (s, sc, sh, mean, rstd, code, g)]
    ds, part = _nan(s.shape, dtype), _nan((blocks, 2, c))
    _ck(lib.mcgen_gated_bwd_stats(*[_p(t) for t in dev], _p(ds), _p(part), blocks, _dt(dtype), n, hw, c, _stream()), 'stats')
    torch.cuda.synchronize()
    ppb = _check_partials(part, pixels, blocks, 'gated_bwd_stats')
    lanes = 256 // (c // 8)
    dz, db, s1, s2 = R.gated_bwd_stats(s, sc, sh, mean, rstd, code, g)
    a64, b64 = s[..., :c].double(), s[..., c:].double()
    q = torch.sigmoid(b64)
    amp = (g.double() * code.double()[:, None, :] * (a64 * sc.double() + sh.double()).clamp_min(0)).abs()
    _assert_within(ds[..., :c], dz, _out_tol(dz, 14 * U32 * dz.abs(), dtype), 'dz')
    _assert_within(ds[..., c:], db, _out_tol(db, 20 * U32 * amp * q, dtype), 'db')
    dgamma, dbeta = _nan((c,)), _nan((c,))
    sums = ops._bwd_sums(part, c, dgamma, dbeta)
    torch.cuda.synchronize()
    xh = (a64 - mean.double()) * rstd.double()
    _assert_within(sums[0], s1, _sum_tol(7, dz.abs().reshape(-1, c).sum(0), s1, ppb, lanes, blocks), 's1')
    _assert_within(sums[1], s2, _sum_tol(10, (dz * xh).abs().reshape(-1, c).sum(0), s2, ppb, lanes, blocks), 's2')
    assert torch.equal(dbeta, sums[0]) and torch.equal(dgamma, sums[1])
    stored = ds.clone()
    _ck(lib.mcgen_gated_bwd_apply(_p(ds), _p(dev[0]), _p(sums), _p(dev[1]), _p(dev[3]), _p(dev[4]), float(pixels), _dt(dtype),
                                  pixels, c, _stream()), 'apply')
    torch.cuda.synchronize()
    inv = R.f32(1.0 / pixels)
    dz_read, sm = stored[..., :c].cpu(), sums.cpu()
    ref = R.bn_apply(dz_read, s[..., :c], sc, mean, rstd, sm[0], sm[1], 1.0 / inv)
    _assert_within(ds[..., :c], ref, _apply_tol(dz_read, s[..., :c], sc, mean, rstd, sm[0], sm[1], inv, ref, dtype), 'da')
    _assert_bits(ds[..., c:].contiguous(), stored[..., c:].contiguous(), 'db after the apply pass')
    dg2, db2 = _nan((c,)), _nan((c,))
    _assert_bits(ops.gated_bwd(dev[0].view(n, 1, hw, 2 * c), *dev[1:6], dev[6].view(n, 1, hw, c), dg2, db2), ds, 'wrapper')
    assert torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)


# (code, pre_relu, y_post, want_gated): the uses of ops.code_bn_bwd in the engines
BN_FLAGS = [(False, False, False, False), (True, False, False, False), (True, True, False, False), (False, True, False, False),
            (True, False, True, False), (True, False, True, True), (False, True, True, True)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c,n,hw', STATS_CASES)
def test_code_bn_bwd(c, n, hw, dtype):
    """mcgen_code_bn_stats, mcgen_bn_bwd_finalize and mcgen_bn_bwd_apply with the wrapper's block rule, for BN_FLAGS;
    ops.code_bn_bwd then gives the same bits.  A flag set that does not use the code, y_post or g_gated does not pass
    them; without pre_relu the shift is a NaN buffer.
    g_gated = g [y_post > 0] is a mask: bit-exact.  dz = g_gated * code is one rounding (exact without a code), doubled; the
    pre-ReLU gate follows the sign of one fma, that of the exact x scale + shift, and is shut at an exact 0.  s1 has terms within u, s2 = sum dz xhat
    within u + 2u + u = 4u, by _sum_tol.  dx is checked from the stored dz and the fp32 sums, bound _apply_tol."""
    ops, lib = _ops(), _lib()
    gen = torch.Generator().manual_seed(c + n + 1)
    pixels = n * hw
    g, x, y = (_randn(gen, n, hw, c, dtype=dtype) for _ in range(3))
    code = torch.randn(n, c, generator=gen)
    sc, sh, mean, rstd = _vec(gen, c), _vec(gen, c, 0.5), _vec(gen, c, 0.5), torch.rand(c, generator=gen) + 0.5
    sc[0], sh[0] = 2.0, -1.0
    x[:, ::3, 0] = 0.5                                                      # x scale + shift = 0 exactly: the pre-ReLU gate is shut
    blocks = _stats_blocks(pixels)
    lanes = 256 // (c // 8)
    gd, xd, yd, coded, scd, shd, meand, rstdd = (t.cuda() for t in (g, x, y, code, sc, sh, mean, rstd))
    inv = R.f32(1.0 / pixels)
    # 4112 pixels x 2048 channels: the two flag sets that between them take every branch of the kernel
    for use_code, pre_relu, use_y, want_gated in (BN_FLAGS if pixels * c < 2 ** 22 else BN_FLAGS[-2:]):
        what = f'code={use_code} pre_relu={pre_relu} y_post={use_y} gated={want_gated}'
        dz_out, part = _nan(x.shape, dtype), _nan((blocks, 2, c))
        gated = _nan(x.shape, dtype) if want_gated else None
        shift_d = shd if pre_relu else _nan((c,))
        _ck(lib.mcgen_code_bn_stats(_p(gd), _p(coded) if use_code else None, _p(xd), _p(meand), _p(rstdd), _p(dz_out), _p(part),
                                    blocks, _dt(dtype), n, hw, c, _p(scd), _p(shift_d), int(pre_relu), _p(yd) if use_y else None,
                                    _p(gated), _stream()), 'code_bn_stats')
        torch.cuda.synchronize()
        ppb = _check_partials(part, pixels, blocks, what)
        dz, s1, s2, gg = R.code_bn_stats(g, code if use_code else None, x, mean, rstd, sc, sh, pre_relu, y if use_y else None)
        if want_gated:
            _assert_bits(gated, torch.where(y > 0, g, torch.zeros_like(g)), what + ': g_gated')
            assert torch.equal(gated.double().cpu(), gg)
        _assert_within(dz_out, dz, _out_tol(dz, (2 * U32 if use_code else 0.0) * dz.abs(), dtype), what + ': dz')
        dgamma, dbeta = _nan((c,)), _nan((c,))
        sums = ops._bwd_sums(part, c, dgamma, dbeta)
        torch.cuda.synchronize()
        xh = (x.double() - mean.double()) * rstd.double()
        _assert_within(sums[0], s1, _sum_tol(1, dz.abs().reshape(-1, c).sum(0), s1, ppb, lanes, blocks), what + ': s1')
        _assert_within(sums[1], s2, _sum_tol(4, (dz * xh).abs().reshape(-1, c).sum(0), s2, ppb, lanes, blocks), what + ': s2')
        assert torch.equal(dbeta, sums[0]) and torch.equal(dgamma, sums[1])
        dx = _nan(x.shape, dtype)
        _ck(lib.mcgen_bn_bwd_apply(_p(dz_out), _p(xd), None, _p(dx), _dt(dtype), pixels, c, _p(sums), float(pixels), _p(scd),
                                   _p(meand), _p(rstdd), _stream()), 'bn_bwd_apply')
        torch.cuda.synchronize()
        dz_read, sm = dz_out.cpu(), sums.cpu()
        ref = R.bn_apply(dz_read, x, sc, mean, rstd, sm[0], sm[1], 1.0 / inv)
        _assert_within(dx, ref, _apply_tol(dz_read, x, sc, mean, rstd, sm[0], sm[1], inv, ref, dtype), what + ': dx')
        dg2, db2 = _nan((c,)), _nan((c,))
        wr = ops.code_bn_bwd(gd, coded if use_code else None, xd, scd, meand, rstdd, dg2, db2, shift=shd if pre_relu else None,
                             pre_relu=pre_relu, y_post=yd if use_y else None, want_gated=want_gated)
        torch.cuda.synchronize()
        if want_gated:
            _assert_bits(wr[1], gated, what + ': wrapper g_gated')
            wr = wr[0]
        _assert_bits(wr, dx, what + ': wrapper dx')
        assert torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)


# ---- 4. the tails, forward ------------------------------------------------------------------------------------------------
def _acr(x, sc, sh, code, res, pre, post):
    n, hw, c = x.shape
    y = _nan(x.shape, x.dtype)
    _ck(_lib().mcgen_affine_code_res(_p(x), _p(sc), _p(sh), _p(code), _p(res), _p(y), _dt(x.dtype), n, hw, c, int(pre), int(post),
                                     _stream()), 'affine_code_res')
    torch.cuda.synchronize()
    return y


def _acr_check(x, sc, sh, code, res, pre, post, dtype, what):
    """z = fma(x, scale, shift) is u |z|, * code another u, + res one more on the sum; ReLUs are exact and 1-Lipschitz:
    |dy| <= 2u |pre_relu?(z) code| + u |y before the last ReLU|, doubled."""
    got = _acr(x.cuda(), sc.cuda(), sh.cuda(), None if code is None else code.cuda(), None if res is None else res.cuda(), pre, post)
    ref = R.affine_code_res(x, sc, sh, code, res, pre, post)
    zk = R.affine_code_res(x, sc, sh, code, None, pre, False)
    last = R.affine_code_res(x, sc, sh, code, res, pre, False)
    _assert_within(got, ref, _out_tol(ref, 2 * (2 * U32 * zk.abs() + U32 * last.abs()), dtype), what)
    return got


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('flags', range(16))
def test_affine_code_res(flags, dtype):
    """The 16 combinations of code x res x pre_relu x post_relu on 3 x 35 pixels, C = 24, with real-valued codes of both
    signs; an unused code or res is not passed at all."""
    use_code, use_res, pre, post = (bool(flags >> i & 1) for i in range(4))
    gen = torch.Generator().manual_seed(flags)
    x, res = _randn(gen, 3, 35, 24, dtype=dtype), _randn(gen, 3, 35, 24, dtype=dtype)
    sc, sh, code = _vec(gen, 24), _vec(gen, 24, 0.5), torch.randn(3, 24, generator=gen)
    got = _acr_check(x, sc, sh, code if use_code else None, res if use_res else None, pre, post, dtype, f'flags {flags:04b}')
    wr = _ops().affine_code_res(x.cuda(), sc.cuda(), sh.cuda(), code.cuda() if use_code else None, res.cuda() if use_res else None,
                                pre, post)
    _assert_bits(wr, got, 'wrapper')


@pytest.mark.parametrize('dtype', DTYPES)
def test_affine_code_res_past_the_grid_cap(dtype):
    """3 x 349 600 pixels at C = 8 (224 vectors past the grid), every flag on."""
    gen = torch.Generator().manual_seed(5)
    x, res = _randn(gen, 3, 349600, 8, dtype=dtype), _randn(gen, 3, 349600, 8, dtype=dtype)
    _acr_check(x, _vec(gen, 8), _vec(gen, 8, 0.5), torch.randn(3, 8, generator=gen), res, True, True, dtype, 'past the cap')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c', [8, 16, 32, 64])
def test_affine_relu_maxpool2(c, dtype):
    """3 images, Ho x Wo = 3 x 5 (input 6 x 10), scales of both signs.  A tenth of the windows has x = (-1 - shift) / scale in
    all four places, i.e. z near -1: the result there is exactly 0.  Elsewhere max(0, fma) is one rounding of the winning
    z: u max |z| over the window, doubled."""
    gen = torch.Generator().manual_seed(c)
    sc, sh = _vec(gen, c), _vec(gen, c, 0.5)
    sc[sc.abs() < 0.1] = 0.5
    assert (sc < 0).any() and (sc > 0).any()
    x = torch.randn(3, 3, 2, 5, 2, c, generator=gen)
    neg = torch.rand(3, 3, 1, 5, 1, c, generator=gen) < 0.1
    x = torch.where(neg, ((-1 - sh) / sc).expand_as(x), x).reshape(3, 6, 10, c).to(dtype)
    y = _nan((3, 3, 5, c), dtype)
    xd, scd, shd = x.cuda(), sc.cuda(), sh.cuda()
    _ck(_lib().mcgen_affine_relu_maxpool2(_p(xd), _p(scd), _p(shd), _p(y), _dt(dtype), 3, 3, 5, c, _stream()), 'pool')
    torch.cuda.synchronize()
    ref = R.affine_relu_maxpool2(x, sc, sh)
    zmax = (x.double() * sc.double() + sh.double()).abs().reshape(3, 3, 2, 5, 2, c).amax(dim=(2, 4))
    _assert_within(y, ref, _out_tol(ref, 2 * U32 * zmax, dtype), f'maxpool C={c}')
    dead = neg.reshape(3, 3, 5, c)
    assert int(dead.sum()) > 0 and bool((ref[dead] == 0).all()) and bool((y.cpu()[dead] == 0).all())
    _assert_bits(_ops().affine_relu_maxpool2(xd, scd, shd), y, 'wrapper')


# ---- 5. losses ------------------------------------------------------------------------------------------------------------
def _bce_case(pixels, c, cp, dtype, gen):
    a = torch.randn(pixels, c, generator=gen) * 8
    t = torch.rand(pixels, c, generator=gen)
    t[torch.rand(pixels, c, generator=gen) < 0.2] = 0.0
    t[torch.rand(pixels, c, generator=gen) < 0.2] = 1.0
    ext = torch.tensor([200.0, -200.0, 100.5, -100.5, 99.5, -99.5, 90.0, -90.0, 40.0, -40.0, 0.0, 17.0])
    for j, tv in enumerate((0.0, 1.0, 0.25)):                               # every extreme against t = 0, 1 and in between
        a.view(-1)[j * 12:(j + 1) * 12] = ext
        t.view(-1)[j * 12:(j + 1) * 12] = tv
    ap, tp = torch.full((pixels, cp), NAN), torch.full((pixels, cp), NAN)
    ap[:, :c], tp[:, :c] = a, t
    return ap.to(dtype), tp


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c,cp', [(3, 8), (8, 8)])
@pytest.mark.parametrize('pixels', [1000, 40000])
def test_bce_logits(pixels, c, cp, dtype):
    """Logits up to +-200 against targets 0, 1 and in between: t min(softplus(-a), 100) + (1 - t) min(softplus(a), 100) hits
    both clamps.  40 000 x 8 elements are 57 856 more than LOSS_BLOCKS x 256: every partial is used and the stride loop
    takes a second trip.
    recon = 1 / (1 + expf(-a)): 5u r (module docstring), doubled, + TINY where expf overflows.
    dlogits = (r - t) gscale: |gscale| (5u r + u |r - t|) + u |d|, doubled, + TINY.
    Loss: L = log1pf(expf(-|a|)) has expf within 2u, which log1p passes on scaled by e / ((1 + e) L) <= 1, and log1pf within
    LOG1P_ULP ulp = 2 LOG1P_ULP u: (2 + 2 LOG1P_ULP) u L.  sp+ = max(a, 0) + L adds u: E+ = (3 + 2 LOG1P_ULP) u sp+;
    sp- = sp+ - a: E- = E+ + u sp-.  min(., 100) is 1-Lipschitz.  term = t m- + (1 - t) m+ adds 3u |term| (1 - t, two
    products, one fma).  A thread adds `trips` terms, the block 8 more (shuffles and waves), the wrapper sums the partials in
    fp64 and rounds once: sum (t E- + (1 - t) E+ + 3u term) + (trips + 8) u sum term + u |S|, doubled.
    Padded channels are never read (NaN) and come out exactly 0 in recon and dlogits."""
    gen = torch.Generator().manual_seed(pixels + c)
    a, t = _bce_case(pixels, c, cp, dtype, gen)
    gs = 0.37
    recon, loss, dl = _ops().bce_logits(a.cuda(), t.cuda(), c, gs, True)
    torch.cuda.synchronize()
    a64, t64 = a[:, :c].double(), t[:, :c].double()
    r, terms, d = R.bce_logits(a64, t64, R.f32(gs))
    for out, name in ((recon, 'recon'), (dl, 'dlogits')):
        assert bool((out[:, c:] == 0).all()), f'{name}: padded channels must be 0'
    _assert_within(recon[:, :c], r, _out_tol(r, 10 * U32 * r + TINY, dtype), 'recon')
    td = 2 * (abs(gs) * (5 * U32 * r + U32 * (r - t64).abs()) + U32 * d.abs()) + TINY
    _assert_within(dl[:, :c], d, _out_tol(d, td, dtype), 'dlogits')
    sp_pos, sp_neg = R.softplus(a64), R.softplus(-a64)
    e_pos = (3 + 2 * LOG1P_ULP) * U32 * sp_pos
    e_neg = e_pos + U32 * sp_neg
    blocks = max(1, min(LOSS_BLOCKS, (pixels * cp + 255) // 256))
    trips = (pixels * cp + blocks * 256 - 1) // (blocks * 256)
    assert trips == (2 if pixels == 40000 else 1)
    s = float(terms.sum())
    tol = 2 * (float((t64 * e_neg + (1 - t64) * e_pos + 3 * U32 * terms).sum()) + (trips + 8) * U32 * s + U32 * s)
    assert abs(float(loss) - s) <= tol, (float(loss), s, tol)
    clamped = (a64.abs() > 100)
    assert float(terms.max()) == 100.0 and int((clamped & (t64 == 0)).sum()) >= 2 and int((clamped & (t64 == 1)).sum()) >= 2
    recon2, loss2, none = _ops().bce_logits(a.cuda(), t.cuda(), c, gs, False)
    assert none is None and torch.equal(loss2, loss)
    _assert_bits(recon2, recon, 'want_grad=False')


def _ce_case(pixels, c, cp, dtype, gen):
    x = torch.randn(pixels, c, generator=gen) * 3
    tgt = torch.randint(0, c, (pixels,), generator=gen)
    x[0] *= 40                                                              # a saturated softmax
    x[1] = 1.25                                                             # all entries equal
    x[2] = x[2] * 40 + 300
    tgt[0], tgt[1], tgt[2], tgt[3] = 0, c - 1, int(x[2].argmax()), int(x[3].argmax())
    if c > 2:
        x[4, 1:c - 1:2] = -INF                                              # -inf entries, away from the target
        tgt[4] = 0
        x[5, :c - 1] = -INF                                                 # a single finite entry
        tgt[5] = c - 1
    if c > 64:
        tgt[6] = 64 + (c - 65) // 2                                         # targets in a lane's second trip
    xp = torch.full((pixels, cp), NAN)
    xp[:, :c] = x
    return xp.to(dtype), tgt


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c,cp', [(10, 16), (20, 24), (64, 64), (65, 72), (512, 512)])
@pytest.mark.parametrize('pixels', [7, 1023])
def test_cross_entropy(pixels, c, cp, dtype):
    """One wave per row, four rows per block: 7 and 1023 rows leave the last block ragged.
    With d_c = x_c - m (m the exact row maximum) and e_c = exp(d_c): the subtraction is u |d_c|, expf 2u, so each term of
    se = sum e_c is within (|d_c| + 2) u e_c; a lane adds ceil(C / 64) terms and the wave 6 more.  logf adds 2u |log se|,
    m + log se one u |lse|, lse - x_t one u |row|:
      T = sum_c e_c (|d_c| + 2) u / se + (ceil(C / 64) + 6) u + 2u |log se| + u |lse|,   |d row| <= 2 (T + u |row|).
    dlogits_c = (expf(x_c - lse) - [c = t]) gscale: the exponent is off by u |x_c - lse| + T, expf adds 2u, the difference
    u, the product u: |gscale| (p_c (u |x_c - lse| + T + 2u) + u |p_c - [c = t]|) + u |d_c|, doubled, + TINY (a saturated
    softmax has entries far below the fp32 range, which come out as 0).  Entries at -inf give p = 0 exactly.  Padded logits are NaN and never read; padded dlogits come out exactly 0."""
    gen = torch.Generator().manual_seed(pixels + c)
    x, tgt = _ce_case(pixels, c, cp, dtype, gen)
    gs = R.f32(1.0 / pixels)
    rows, dl = _nan((pixels,)), _nan((pixels, cp), dtype)
    xd, td = x.cuda(), tgt.cuda()
    _ck(_lib().mcgen_cross_entropy(_p(xd), _p(td), _p(rows), _p(dl), 1.0 / pixels, _dt(dtype), pixels, c, cp, _stream()), 'ce')
    torch.cuda.synchronize()
    x64 = x[:, :c].double()
    r_ref, d_ref = R.cross_entropy(x64, tgt, gs)
    m = x64.max(-1, keepdim=True).values
    dc = x64 - m
    e = torch.exp(dc)
    se = e.sum(-1)
    lse = m.view(-1) + torch.log(se)
    t_row = (torch.where(e > 0, e * (dc.abs() + 2), torch.zeros_like(e)).sum(-1) / se + (math.ceil(c / 64) + 6)
             + 2 * torch.log(se).abs() + lse.abs()) * U32
    _assert_within(rows, r_ref, 2 * (t_row + U32 * r_ref.abs()), 'loss rows')
    p = torch.exp(x64 - lse[:, None])
    onehot = torch.nn.functional.one_hot(tgt, c).double()
    expo = torch.where(p > 0, p * (U32 * (x64 - lse[:, None]).abs() + t_row[:, None] + 2 * U32), torch.zeros_like(p))
    t32 = 2 * (gs * (expo + U32 * (p - onehot).abs()) + U32 * d_ref.abs()) + TINY
    _assert_within(dl[:, :c], d_ref, _out_tol(d_ref, t32, dtype), 'dlogits')
    assert bool((dl[:, c:] == 0).all()), 'padded dlogits must be 0'
    rows2, dl2 = _ops().cross_entropy(xd, td, c, True)
    rows3, none = _ops().cross_entropy(xd, td, c, False)
    assert none is None and torch.equal(rows2, rows) and torch.equal(rows3, rows)
    _assert_bits(dl2[:, :c].contiguous(), dl[:, :c].contiguous(), 'wrapper dlogits')


# ---- 6. arg-min -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c,cp', [(1, 8), (33, 40), (64, 64), (100, 104), (512, 512)])
def test_argmin_channels(c, cp, dtype):
    """203 rows (the last block holds 3).  Rows with a duplicated minimum in one lane (c and c + 64), in two lanes, 0.0
    against -0.0 in both orders, rows that are all +inf, all -inf, all NaN, that hold -inf twice, one or several NaN, and
    +inf everywhere but one entry; the rest random (in bf16 ties are then the common case).  The result equals torch.argmin
    on the same values and the fp64 first-minimum reference, and lies in [0, C).  Padding is NaN and must not win."""
    gen = torch.Generator().manual_seed(c)
    pixels = 203
    x = torch.randn(pixels, c, generator=gen)
    hi, mid = c - 1, c // 2
    x[0] = INF
    x[1] = NAN
    x[2] = -INF
    x[3] = INF; x[3, hi] = 3e38
    x[4, mid] = NAN; x[4, hi] = NAN
    x[5, mid] = -INF; x[5, hi] = -INF
    x[6, hi] = NAN; x[6, 0] = -INF
    x[7] = 0.0; x[7, hi] = -0.0
    x[8] = -0.0; x[8, mid] = 0.0
    x[9] = 1.0; x[9, hi] = 0.0; x[9, mid] = -0.0
    x[10, mid] = -9.0; x[10, hi] = -9.0                                     # two lanes (or one, when C = 1)
    if c > 64:
        x[11, 7] = -9.0; x[11, 71] = -9.0                                   # one lane, two trips
        x[12, 71] = -9.0; x[12, 8] = -9.0                                   # the later trip of a lower lane against a higher lane
        x[13] = INF; x[13, 70] = 5.0
        x[14, 70] = NAN; x[14, 6] = 0.0
    xp = torch.full((pixels, cp), NAN)
    xp[:, :c] = x
    xp = xp.to(dtype)
    got = _ops().argmin_channels(xp.cuda(), c).cpu()
    vals = xp[:, :c].float()
    ref = torch.argmin(vals, -1)
    assert torch.equal(R.argmin(vals), ref)
    assert got.dtype == torch.int64 and int(got.min()) >= 0 and int(got.max()) < c
    assert torch.equal(got, ref), (got - ref).nonzero().view(-1).tolist()[:10]
    if dtype == torch.bfloat16 and c >= 100:
        srt = vals[20:].sort(-1).values
        assert int((srt[:, 0] == srt[:, 1]).sum()) > 0                      # random rows with a tied minimum exist


# ---- 7. the VQ training step and the tanh + MSE loss ----------------------------------------------------------------------
def _vq_inputs(d, k, p, gen):
    emb = torch.randn(d, k, generator=gen)
    codes = torch.randint(0, k, (p,), generator=gen)
    codes[torch.randperm(p, generator=gen)[:p // 3]] = 3                    # one popular code
    codes[codes == 5] = 6                                                   # one code never hit
    codes[0] = k - 1
    if p > 1:
        codes[p - 1] = 0
    feat = torch.full((p, d + 8), NAN)
    feat[:, :d] = emb[:, codes].t() + 0.1 * torch.randn(p, d, generator=gen)
    cs0 = torch.rand(k, generator=gen) * 4 + 0.01
    return emb, codes, feat, cs0, emb * (cs0 + 1e-5)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('k', [64, 512])
@pytest.mark.parametrize('d', [16, 24, 32, 40, 48, 56])
def test_vq_step(d, k, dtype):
    """P = 1, 100, 128, 1000 pixels (a lone pixel, a short chunk, a full one, seven full chunks and a tail of 104), feature rows
    of pitch D + 8 with NaN padding, codes 0 and K - 1 in use, one code unused; q and g in `dtype`.  D = 24, 40, 56 run the
    tail-wave branch of vq_stats.  Two runs from the same state give the same bits.
    q = E[:, code] is a copy (rounded once for bf16) and the counts are small integers: exact.
    g = coef (f - q): two roundings, doubled.
    diff = sum (f - q)^2 / (P D): a term is within 3u; a thread adds 8 ceil(VQ_PC (D / 8) / 256) of them and the block 8 more,
    vq_count adds the chunks one by one, the scaling rounds twice: (3 + n + 8 + chunks + 2) u diff, doubled.
    cluster_size = decay cs0 + (1 - decay) count: 3u (|decay cs0| + |(1 - decay) count|), doubled.
    embedding_mean: a slab entry adds at most VQ_PC features (the products with the 0 / 1 mask are exact), vq_refresh adds
    the chunks: (VQ_PC + chunks) u A with A = |f|^T onehot; then em = decay m0 + (1 - decay) s: (1 - decay) times that
    + 3u (|decay m0| + |(1 - decay) s|), doubled.
    embedding = em / cs', cs' = (cs + eps) / (n + K eps) n, all positive: n is K <= 1024 values in a chain of 1 + 6 + 16
    additions over values within 3u (26u), the denominator 28u, cs + eps 4u, the division 2u, the product with n 27u:
    |d cs'| <= 61u cs', so |d e| <= |d em| / cs' + 63u |e|, doubled."""
    ops = _ops()
    decay, omd, eps, commit = R.f32(0.99), R.f32(1.0 - 0.99), R.f32(1e-5), 0.25
    assert d <= VQ_DMAX and d % 16 in (0, 8) and k % VQ_KT == 0
    for p in (1, 100, 128, 1000):
        gen = torch.Generator().manual_seed(d + k + p)
        emb, codes, feat, cs0, mean0 = _vq_inputs(d, k, p, gen)
        coef = commit * 2 / (p * d)
        chunks = (p + VQ_PC - 1) // VQ_PC
        runs = []
        for _ in range(2):
            e_d, cs_d, em_d = emb.cuda(), cs0.cuda(), mean0.cuda()
            q, g, diff, counts = ops.vq_step(feat.cuda(), codes.cuda(), e_d, d, dtype, coef=coef, want_grad=True, train=True,
                                             cluster_size=cs_d, embedding_mean=em_d, decay=0.99, eps=1e-5, want_counts=True)
            torch.cuda.synchronize()
            runs.append([t.cpu() for t in (q, g, diff, counts, cs_d, em_d, e_d)])
        for a, b in zip(*runs):
            assert torch.equal(a, b), 'reruns differ'
        q, g, diff, counts, cs, em, e = runs[0]
        what = f'D={d} K={k} P={p}'
        f64 = feat[:, :d].double()
        r = R.vq_step(f64, codes, emb, cs0, mean0, decay, omd, eps, commit)
        assert r['counts'][k - 1] >= 1 and (p == 1 or r['counts'][0] >= 1) and r['counts'][5] == 0
        _assert_bits(q, r['q'].to(dtype), what + ': q')
        assert torch.equal(counts.double(), r['counts']), what + ': counts'
        g_ref = R.f32(coef) * (f64 - r['q'])
        _assert_within(g, g_ref, _out_tol(g_ref, 4 * U32 * g_ref.abs(), dtype), what + ': g')
        n_thread = 8 * math.ceil(VQ_PC * (d // 8) / 256)
        dref = float(r['diff'])
        assert abs(float(diff) - dref) <= 2 * (3 + n_thread + 8 + chunks + 2) * U32 * dref, (what, float(diff), dref)
        t_cs = 3 * U32 * ((decay * cs0.double()).abs() + omd * r['counts'])
        _assert_within(cs, r['cs'], 2 * t_cs, what + ': cluster_size')
        a_abs = f64.abs().t() @ r['onehot']
        s_sum = f64.t() @ r['onehot']
        t_em = omd * (VQ_PC + chunks) * U32 * a_abs + 3 * U32 * ((decay * mean0.double()).abs() + (omd * s_sum).abs())
        _assert_within(em, r['em'], 2 * t_em, what + ': embedding_mean')
        n_cs = r['cs'].sum()
        cs_out = (r['cs'] + eps) / (n_cs + k * eps) * n_cs
        _assert_within(e, r['e'], 2 * (t_em / cs_out.abs() + 63 * U32 * r['e'].abs()), what + ': embedding')


@pytest.mark.parametrize('dtype', DTYPES)
def test_vq_step_eval_touches_no_statistics(dtype):
    """train = 0 with every buffer passed: q, g and diff as in training; the slabs stay NaN, cluster_size, embedding_mean,
    embedding, counts and the scratch keep their bits.  D = 40 (tail wave), K = 128, P = 300."""
    lib = _lib()
    d, k, p = 40, 128, 300
    gen = torch.Generator().manual_seed(9)
    emb, codes, feat, cs0, mean0 = _vq_inputs(d, k, p, gen)
    chunks = lib.mcgen_vq_chunks(p)
    assert chunks == (p + VQ_PC - 1) // VQ_PC
    coef = R.f32(0.5 / (p * d))
    fd, cd, ed, csd, emd = feat.cuda(), codes.cuda(), emb.cuda(), cs0.cuda(), mean0.cuda()
    q, g = _nan((p, d), dtype), _nan((p, d), dtype)
    slab, cslab, dpart, diff = _nan((chunks, d, k)), _nan((chunks, k)), _nan((chunks,)), _nan(())
    counts, scratch = _nan((k,)), _nan((k,))
    _ck(lib.mcgen_vq_stats(_p(fd), _p(cd), _p(ed), _p(q), _p(g), _p(slab), _p(cslab), _p(dpart), coef, _dt(dtype), p, d, d + 8, k, 0,
                           _stream()), 'vq_stats')
    _ck(lib.mcgen_vq_update(_p(slab), _p(cslab), _p(dpart), p, d, k, 0.99, 0.01, 1e-5, _p(csd), _p(emd), _p(ed), _p(counts),
                            _p(scratch), _p(diff), 0, _stream()), 'vq_update')
    torch.cuda.synchronize()
    for t in (slab, cslab, counts, scratch):
        assert bool(torch.isnan(t).all())
    assert torch.equal(ed.cpu(), emb) and torch.equal(csd.cpu(), cs0) and torch.equal(emd.cpu(), mean0)
    f64 = feat[:, :d].double()
    r = R.vq_step(f64, codes, emb, cs0, mean0, 0.99, 0.01, 1e-5, 0.25)
    _assert_bits(q, r['q'].to(dtype), 'q')
    g_ref = coef * (f64 - r['q'])
    _assert_within(g, g_ref, _out_tol(g_ref, 4 * U32 * g_ref.abs(), dtype), 'g')
    n_thread = 8 * math.ceil(VQ_PC * (d // 8) / 256)
    assert abs(float(diff) - float(r['diff'])) <= 2 * (3 + n_thread + 8 + chunks + 2) * U32 * float(r['diff'])
    q2, none, diff2, none2 = _ops().vq_step(fd, cd, ed, d, dtype)
    assert none is None and none2 is None and torch.equal(diff2, diff)
    _assert_bits(q2, q, 'wrapper q')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('pixels', [1000, 262500])
def test_mse_tanh(pixels, dtype):
    """C = 3 of Cp = 8, |x| up to 20 (tanh saturates to 1 in fp32 from about 9), NaN in the padding of x and of the target.
    262 500 pixels are 356 more vectors of 8 than LOSS_BLOCKS x 256: every partial and a second trip.
    decoded r = tanhf(x): TANH_ULP ulp = 2 TANH_ULP u |r|, doubled.  e = r - t: E = 2 TANH_ULP u |r| + u |e|.
    sse: a term e^2 is within 2 |e| E + u e^2; a thread adds 3 `trips` terms and the block 8 more, the wrapper sums the
    partials in fp64 and rounds once: sum (2 |e| E + u e^2) + (3 trips + 8 + 1) u sse, doubled.
    dx = gscale e (1 - r^2): r^2 is within (4 TANH_ULP + 1) u r^2, 1 - r^2 adds u: D = (4 TANH_ULP + 1) u r^2 + u (1 - r^2);
    |d dx| <= |gscale| (E (1 - r^2) + |e| D) + 2u |dx|, doubled.
    Padded channels come out exactly 0 in decoded and dx."""
    gen = torch.Generator().manual_seed(pixels)
    c, cp, gs = 3, 8, 2.0 / (pixels * 3)
    x = torch.randn(pixels, c, generator=gen) * 2
    x[:7, 0] = torch.tensor([20.0, -20.0, 12.0, -9.5, 1e-4, 0.0, -1e-3])
    x[7:, 1] *= 4
    x = x.clamp(-20, 20)
    t = torch.rand(pixels, c, generator=gen) * 2 - 1
    xp, tp = torch.full((pixels, cp), NAN), torch.full((pixels, cp), NAN)
    xp[:, :c], tp[:, :c] = x, t
    xp = xp.to(dtype)
    dec, sse, dx = _ops().mse_tanh(xp.cuda(), tp.cuda(), c, gs, True)
    torch.cuda.synchronize()
    x64, t64 = xp[:, :c].double(), t.double()
    assert float(x64.abs().max()) == 20.0
    r, s_ref, d_ref = R.mse_tanh(x64, t64, R.f32(gs))
    for out, name in ((dec, 'decoded'), (dx, 'dx')):
        assert bool((out[:, c:] == 0).all()), f'{name}: padded channels must be 0'
    tu = 2 * TANH_ULP * U32
    _assert_within(dec[:, :c], r, _out_tol(r, 2 * tu * r.abs(), dtype), 'decoded')
    e = r - t64
    err_e = tu * r.abs() + U32 * e.abs()
    blocks = max(1, min(LOSS_BLOCKS, (pixels * cp // 8 + 255) // 256))
    trips = (pixels + blocks * 256 - 1) // (blocks * 256)
    assert trips == (2 if pixels == 262500 else 1)
    s = float(s_ref)
    tol = 2 * (float((2 * e.abs() * err_e + U32 * e * e).sum()) + (3 * trips + 9) * U32 * s)
    assert abs(float(sse) - s) <= tol, (float(sse), s, tol)
    one_m = 1 - r * r
    err_1m = (2 * tu + U32) * r * r + U32 * one_m
    t32 = 2 * (abs(gs) * (err_e * one_m + e.abs() * err_1m) + 2 * U32 * d_ref.abs())
    _assert_within(dx[:, :c], d_ref, _out_tol(d_ref, t32, dtype), 'dx')
    dec2, sse2, none = _ops().mse_tanh(xp.cuda(), tp.cuda(), c, gs, False)
    assert none is None and torch.equal(sse2, sse)
    _assert_bits(dec2, dec, 'want_grad=False')
