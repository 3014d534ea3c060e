"""The label-conditioning kernels of the conditional baselines one at a time, in fp32 and bf16, at the smallest shapes that
reach each path: csrc/cgan_ops.hip, csrc/cvae_ops.hip, csrc/cpixelcnn_ops.hip, csrc/cglow_ops.hip, and the per-sample-row
path of the incremental sampler (mcgen_cpx_sample_row / _col) through ConditionalGatedPixelCNN.sample.

Conventions, those of test_pixel_vq_kernels_gpu.py (whose helpers are imported): every reference is float64 on the CPU
(tests/cond_ops_ref.py, checked against torch autograd in test_cond_ops_ref_cpu.py) from exactly the values the kernel
read; destinations and pads start as NaN, pads the op writes must be exactly 0; inputs carry NaN wherever the op must not
read (channels at or beyond C of padded rows, weight columns outside the embedding's, table entries of absent labels, the
gap of a pitch); copies, gathers and zero fills are compared bit for bit; every kernel is run twice and must return the
same bits (_twice).  Every other bound is per element and derived with u = 2^-24: a correctly rounded fp32 operation is
within u, expf and division within 2u, the sigmoid within 5u q, a chain of n fp32 additions within n u sum|terms|, a bf16
store adds 2^-8 |v| (_out_tol).  "mag" is the reference's sum of the magnitudes of an output's terms.  Bounds are doubled
for second-order terms.  A result below the smallest normal fp32 (TINY) may be flushed: where a sigmoid saturates the
bound has a floor of TINY times the factor it multiplies.  No accuracy assumption beyond that file's is made.

Per kernel: the path each case reaches, and its bound.

mcgen_cgan_embed_bwd (embed_bwd_kernel; fp32 only).  N = 1 / 1024 / 1025 / 2049: one ragged chunk, one full chunk, the
  second trip of the LDS label loop with a chunk of 1, a third trip.  (E, M) = (1, 1) / (8, 3) / (256, 5): one thread, a
  ragged workgroup, several workgroups.  Labels -1, M and 2^40 (no row), mode 0 held by the first and the last sample
  (both chunks).  ld = E + 8 with NaN in the gap; ld = E through the wrapper.  accumulate onto a non-zero gradient.
  Bound: mode m adds count_m (+ 1 accumulating) terms: 2 (count_m + 1) u mag.
mcgen_cgan_gen_input, mcgen_cgan_dis_input, mcgen_cvae_enc_input.  L + E and C + E = 4 (below one vector of 8), 259 / 257
  / 263 (E = 256), M = 1, input pitch Cpi > Cimg with NaN in the pad, HW = 1, and for enc_input 24 x 24 x 40 channels =
  2880 vectors, past the 8 x 256 of one grid pass.  gen_input, enc_input's embedding channels and dis_input at sigma = 1
  are copies: bit-exact.  dis_input at sigma = 1.7: w * (1 / sigma), 3u, doubled.  enc_input's image channels:
  (x + 1) * 0.5 is one rounding, doubled.
mcgen_cgan_lin_dembed.  (E, C0) = (1, 4): S = 1024 slices of a 64-long range, 960 of them empty; (256, 4): S = 4;
  (32, 24): the workload; (8, 1): 16 columns in 128 slices.  col0 > 0 and in_features > col0 + E with NaN outside the
  columns.  Bound: products u, a slice adds per = ceil(16 C0 / S) terms, S slices: 2 (1 + per + S) u mag.
mcgen_cgan_dis_window_sums.  W = 2 (no interior column), H != W, C > 256 (second trip of the channel stride), Cp > C.  The
  first and last columns are copies (bit-exact), the interior a chain of W - 2.
mcgen_cgan_dis_dembed.  C = 8 / 24 / 96 / 320 / 1024: G = 128 / 42 / 10 / 3 / 1 pixel groups, idle threads for 24, 96 and
  320; E = 1 / 32 / 256; Cimg = 0 / 1 / 3; HWq = 1 on the 2 x 2 maps; Cpq > C.  Bound: the longest chain is interior
  columns (W), interior rows (H), cells of a tap (9) or pooled pixels (HWq / G + G), the weight w * (1 / sigma) (3u), the
  product, a slice of per = ceil(10 C / S) and S slices: 2 (max(W + H + 9, HWq / G + G) + 4 + per + S) u mag.  C = 1032 is
  refused with the documented text and writes nothing.
mcgen_cvae_enc_dembed.  The same maps with C = 8 / 24 / 960 (960: the 64 KB dynamic LDS request), E = 1 / 32 / 256;
  bound as above with 16 taps and no shortcut.  C = 968 is refused.
mcgen_cvae_latent_fwd / _bwd.  L = 1 / 16 / 255 / 257 (one live thread, most threads idle, a ragged full pass, a second
  trip), ldm > 2L with NaN in the gap, Cp > L + E, Cq > 2L, E = 0 with de = NULL, logvar over [-30, 20].  mu, logvar, the
  embedding columns and de are copies.  z = mu + eps expf(lv / 2): 3u |eps sd| + u |z|.  kl: a thread adds 4 terms per
  column, the tree 8 levels, expf 2u: 2 (4 ceil(L / 256) + 10) u kl_mag.  One sample has logvar = 200: its kl and kld
  are +inf (not NaN), its z is +-inf, the other samples stay finite.  dmu: u |mu inv| + u |dmu|; dlogvar: 4u |a| +
  (2u e^lv + u |e^lv - 1|) inv / 2 + u |b| + u |dlogvar|.
mcgen_cglow_prior / _bwd.  C2 = 2 / 8 / 258 / 520 (one thread, a second workgroup of the parameter kernel, the second and
  third trip of the channel stride), N = 1 / 3 / 1025 (second LDS label chunk), HW = 1, dw_p absent / 7 / 20001 elements
  (past the 64 x 256 of the zero fill), s_p and s_e up to +-3.  expf(3 s) has a rounded argument: (3 |s| + 3) u.  prior:
  (3 |s| + 4) u per term + u |h|.  dh: a chain of HW.  The parameter gradients are checked from the dh the kernel wrote:
  chains of N, 2 (N + 3 |s| + 8) u mag.  dw_e from the kernel's own rows, as embed_bwd.  dw_p is exactly 0.
mcgen_cpx_gate_stats, _gated_fwd, _gated_bwd_stats / _apply.  C = 8 / 2048 (lanes = 256 / 1), C = 24 forward only
  (statistics refused).  (N, HW) = (3, 35): 105 pixels in 6 blocks of 18, the last ragged (15), blocks straddle the
  images off the 16-pixel grid; (7, 46): 322 pixels in 20 blocks of 17, block 18 ragged (16) and block 19 empty.  Labels -1 and M + 3 are clamped.
  Gate inputs b + e_b at +-100 in two channels, z of both signs and exactly 0 in channel 0.  x = s + e is one rounding.
  One launch of three jobs of unequal N, HW, C and blocks equals the single launches bit for bit and leaves the rows of
  a shorter job's partials past its blocks untouched.  Bounds: _gate_errs and the docstrings below.
mcgen_cpx_embed_bwd, mcgen_cpx_gather_rows.  M = 1, N = 1, M * C2 and L * N * C2 above the 4096 x 256 of one grid pass.
mcgen_cpx_code_embed_bwd.  P = 1 / 255 / 257 / 513, C = 1 / 40 / 256, Cp = C + 8 with NaN in the pad, a chunk of 256 equal
  codes, chunks without a match, K = 1, codes outside [0, K).  The code and dx buffers run on past P with a matching code
  and NaN rows.  Bound: 2 count_k u mag.
Conditional sampler.  models.cpixelcnn() at hidden 128, 15 layers, 512 codes, 1623 modes, N = 37 on 8 x 8 and 4 x 8,
  labels with the first and the last mode, under the bounds of test_pixelcnn_sample_gpu.py."""
import math

import pytest
import torch

import cond_ops_ref as R
import pixel_ops_ref as PR
from test_pixel_vq_kernels_gpu import (DTYPES, NAN, TINY, U32, _assert_bits, _assert_within, _check_partials, _ck, _dt, _lib,
                                       _nan, _ops, _out_tol, _p, _randn, _stream, _vec)

pytestmark = pytest.mark.gpu

INF = float('inf')
F64 = torch.float64
GRID_ITEMS = 4096 * 256     # cpixelcnn_ops.hip grid_for: the grid-stride loops take a second trip above this
LDS_LABELS = 1024           # embed_bwd_kernel / prior_param_bwd_kernel: labels per LDS chunk
FAR = 2 ** 40               # a label no int32 holds


def _twice(fn):
    """Run fn (-> tensor or tuple of tensors, freshly allocated) twice: the same bits both times; returns the first."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        if x is not None:
            xv, yv = x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)
            assert torch.equal(xv, yv), 'a rerun changed bits'
    return a


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _labels(gen, n, m):
    """Random labels in [0, M) with -1, M and 2^40 at samples 1 .. 3 and mode 0 at the first and the last sample."""
    lab = torch.randint(0, m, (n,), generator=gen)
    lab[0] = lab[-1] = 0
    if n >= 4:
        lab[1], lab[2], lab[3] = -1, m, FAR
    return lab


def _inside(lab, m):
    return (lab >= 0) & (lab < m)


def _poison_columns(w, lab):
    """[E, M] table: NaN in the columns of modes no label reads."""
    w = w.clone()
    absent = torch.ones(w.shape[1], dtype=torch.bool)
    absent[lab[_inside(lab, w.shape[1])]] = False
    w[:, absent] = NAN
    return w


def _padded(x, cp, dtype):
    """x [..., C] -> [..., cp] in dtype on the device, NaN in the channels at and beyond C."""
    out = torch.full(x.shape[:-1] + (cp,), NAN, dtype=dtype)
    out[..., :x.shape[-1]] = x.to(dtype)
    return out.cuda()


def _refused(rc, text):
    from mcgen_amd._lib import load
    assert rc != 0
    msg = load().mcgen_last_error().decode()
    assert text in msg, msg


# ---- 1. mcgen_cgan_embed_bwd ------------------------------------------------------------------------------------------
def _embed_bwd(de, ld, lab, dw, n, e, m, acc):
    _ck(_lib().mcgen_cgan_embed_bwd(_p(de), ld, _p(lab), _p(dw), n, e, m, int(acc), _stream()), 'cgan_embed_bwd')
    torch.cuda.synchronize()
    return dw


def _embed_bwd_tol(lab, m, mag, acc):
    cnt = torch.bincount(lab[_inside(lab, m)], minlength=m).double()
    return 2 * (cnt + (1 if acc else 0)) * U32 * mag


@pytest.mark.parametrize('e,m', [(1, 1), (8, 3), (256, 5)])
@pytest.mark.parametrize('n', [1, 1024, 1025, 2049])
def test_cgan_embed_bwd(n, e, m):
    gen = _gen(n + e)
    lab = _labels(gen, n, m)
    de = torch.randn(n, e, generator=gen)
    base = torch.randn(e, m, generator=gen)
    if n > LDS_LABELS:
        assert lab[0] == lab[-1] == 0                                      # a mode with samples in the first and the last chunk
    ded, labd = _padded(de, e + 8, torch.float32), lab.cuda()
    for acc in (False, True):
        got = _twice(lambda: _embed_bwd(ded, e + 8, labd, base.cuda() if acc else _nan((e, m)), n, e, m, acc))
        ref, mag = R.embed_bwd(de, lab, m, base if acc else None)
        _assert_within(got, ref, _embed_bwd_tol(lab, m, mag, acc), f'embed_bwd N={n} E={e} M={m} accumulate={acc}')
        if not acc:
            dense = _nan((e, m))
            _ops().cgan_embed_bwd(de.cuda(), labd, dense)
            _assert_bits(dense, got, 'wrapper, ld = E')


# ---- 2. the three input builders ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,lat,e,m', [(5, 3, 1, 1), (4, 7, 256, 3), (3, 128, 32, 10)])
def test_cgan_gen_input(n, lat, e, m, dtype):
    gen = _gen(lat + e)
    lab = _labels(gen, n, m)
    z, w = torch.randn(n, lat, generator=gen), _poison_columns(torch.randn(e, m, generator=gen), lab)
    cp = (lat + e + 7) // 8 * 8 + 8
    zd, wd, labd = z.cuda(), w.cuda(), lab.cuda()

    def run():
        out = _nan((n, cp), dtype)
        _ck(_lib().mcgen_cgan_gen_input(_p(zd), _p(wd), _p(labd), _p(out), _dt(dtype), n, lat, e, m, cp, _stream()), 'gen_input')
        return out
    got = _twice(run)
    ref = torch.zeros(n, cp, dtype=F64)
    ref[:, :lat + e] = R.gen_input(z, w, lab)
    _assert_bits(got, ref.to(dtype), f'gen_input {(n, lat, e, m)}')
    wr = _ops().cgan_gen_input(zd, wd, labd, dtype)
    _assert_bits(wr.reshape(n, -1), ref[:, :wr.shape[-1]].to(dtype).contiguous(), 'wrapper')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,hw,cimg,cpi,e,m', [(3, 6, 3, 8, 1, 1), (2, 1, 3, 3, 256, 4), (4, 35, 1, 8, 32, 10)])
def test_cgan_dis_input(n, hw, cimg, cpi, e, m, dtype):
    gen = _gen(hw + e)
    lab = _labels(gen, n, m)
    img, w = _randn(gen, n, hw, cimg, dtype=dtype), _poison_columns(torch.randn(e, m, generator=gen), lab)
    cp = (cimg + e + 7) // 8 * 8 + 8
    imgd, wd, labd = _padded(img, cpi, dtype), w.cuda(), lab.cuda()
    for sigma in (1.0, 1.7):
        sg = torch.tensor([sigma])
        sgd = sg.cuda()

        def run():
            out = _nan((n, hw, cp), dtype)
            _ck(_lib().mcgen_cgan_dis_input(_p(imgd), _p(wd), _p(sgd), _p(labd), _p(out), _dt(dtype), n, hw, cimg, cpi, e, m, cp,
                                            _stream()), 'dis_input')
            return out
        got = _twice(run)
        ref = torch.zeros(n, hw, cp, dtype=F64)
        ref[..., :cimg + e] = R.dis_input(img, w, float(sg), lab)
        what = f'dis_input {(n, hw, cimg, cpi, e, m)} sigma={sigma}'
        if sigma == 1.0:
            _assert_bits(got, ref.to(dtype), what)
        else:
            _assert_bits(got[..., :cimg].contiguous(), img.to(dtype), what + ': image')
            assert bool((got[..., cimg + e:] == 0).all()), what + ': pad'
            _assert_within(got, ref, _out_tol(ref, 6 * U32 * ref.abs(), dtype), what)
    wr = _ops().cgan_dis_input(imgd.view(n, 1, hw, cpi), cimg, wd, sgd, labd)
    _assert_bits(wr.reshape(n, hw, -1), got[..., :wr.shape[-1]].contiguous(), 'wrapper')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,c,h,wd_,e,m', [(3, 3, 2, 3, 1, 1), (2, 1, 1, 1, 256, 5), (2, 3, 24, 24, 32, 10)])
def test_cvae_enc_input(n, c, h, wd_, e, m, dtype):
    gen = _gen(h + e)
    lab = _labels(gen, n, m) if n >= 3 else torch.tensor([m - 1, -1])
    img = torch.rand(n, c, h, wd_, generator=gen) * 2 - 1
    w = _poison_columns(torch.randn(e, m, generator=gen), lab)
    hw, cp = h * wd_, (c + e + 7) // 8 * 8 + 8
    if h == 24:
        assert hw * (cp // 8) > 8 * 256 and (hw * (cp // 8)) % 256                  # a ragged second grid pass
    imgd, wdev, labd = img.cuda(), w.cuda(), lab.cuda()

    def run():
        out = _nan((n, hw, cp), dtype)
        _ck(_lib().mcgen_cvae_enc_input(_p(imgd), _p(wdev), _p(labd), _p(out), _dt(dtype), n, hw, c, e, m, cp, _stream()), 'enc_input')
        return out
    got = _twice(run)
    ref = torch.zeros(n, hw, cp, dtype=F64)
    ref[..., :c + e] = R.enc_input(img, w, lab)
    what = f'enc_input {(n, c, h, wd_, e, m)}'
    _assert_bits(got[..., c:].contiguous(), ref[..., c:].to(dtype).contiguous(), what + ': embedding and pad')
    _assert_within(got, ref, _out_tol(ref, 2 * U32 * ref.abs(), dtype), what)
    wr = _ops().cvae_enc_input(imgd, wdev, labd, dtype)
    _assert_bits(wr.reshape(n, hw, -1), got[..., :wr.shape[-1]].contiguous(), 'wrapper')


# ---- 3. mcgen_cgan_lin_dembed ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('e,c0', [(1, 4), (256, 4), (32, 24), (8, 1)])
def test_cgan_lin_dembed(e, c0, dtype):
    gen = _gen(e + c0)
    n, col0 = 3, 5
    inf = col0 + e + 3
    dlin = _randn(gen, n, 4, 4, c0, dtype=dtype)
    w = torch.full((16 * c0, inf), NAN)
    w[:, col0:col0 + e] = torch.randn(16 * c0, e, generator=gen)
    dd, wd = dlin.cuda(), w.cuda()

    def run():
        out = _nan((n, e))
        _ck(_lib().mcgen_cgan_lin_dembed(_p(dd), _p(wd), _p(out), _dt(dtype), n, c0, inf, col0, e, _stream()), 'lin_dembed')
        return out
    got = _twice(run)
    ref, mag = R.lin_dembed(dlin, torch.nan_to_num(w), col0, e)
    s = 1024 // e
    per = (16 * c0 + s - 1) // s
    if e == 1:
        assert per * (s - 1) > 16 * c0                                             # most slices are empty
    _assert_within(got, ref, 2 * (1 + per + s) * U32 * mag, f'lin_dembed E={e} C0={c0}')
    _assert_bits(_ops().cgan_lin_dembed(dd, wd, col0, e), got, 'wrapper')


# ---- 4. window sums and the two embedding input gradients that read them --------------------------------------------------
def _window_sums(dc1, c):
    n, h, w, cp = dc1.shape
    part = _nan((n, h, 3, c))
    _ck(_lib().mcgen_cgan_dis_window_sums(_p(dc1), _p(part), _dt(dc1.dtype), n, h, w, c, cp, _stream()), 'window_sums')
    return part


def _check_window_sums(part, x, what):
    """part [N, H, 3, C] against x [N, H, W, C] (the values read): first / last column are copies, the interior is a chain of
    W - 2 additions."""
    w = x.shape[2]
    _assert_bits(part[:, :, 0].contiguous(), x[:, :, 0].float().contiguous(), what + ': first column')
    _assert_bits(part[:, :, 2].contiguous(), x[:, :, -1].float().contiguous(), what + ': last column')
    mid = x[:, :, 1:-1].double()
    _assert_within(part[:, :, 1], mid.sum(2), 2 * max(w - 2, 0) * U32 * mid.abs().sum(2), what + ': interior')
    if w == 2:
        assert bool((part[:, :, 1] == 0).all()), what + ': no interior column'


DEMBED_MAPS = [(2, 2, 8, 1, 0), (2, 2, 8, 256, 1), (4, 6, 24, 32, 3), (6, 4, 96, 256, 1), (2, 2, 1024, 32, 3), (4, 4, 320, 1, 1)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('h,w,c,e,cimg', DEMBED_MAPS)
def test_cgan_dis_dembed(h, w, c, e, cimg, dtype):
    gen = _gen(h * w + c + e)
    n, cin, hwq = 2, cimg + e + 1, (h // 2) * (w // 2)
    dc1, dy = _randn(gen, n, h, w, c, dtype=dtype), _randn(gen, n, h // 2, w // 2, c, dtype=dtype)
    w1, wsc = torch.full((c, cin, 3, 3), NAN), torch.full((c, cin), NAN)
    w1[:, cimg:cimg + e] = torch.randn(c, e, 3, 3, generator=gen)
    wsc[:, cimg:cimg + e] = torch.randn(c, e, generator=gen)
    s1, ssc = torch.tensor([1.7]), torch.tensor([0.6])
    dc1d, dyd = _padded(dc1, c + 8, dtype), _padded(dy, c + 8, dtype)
    w1d, wscd, s1d, sscd = w1.cuda(), wsc.cuda(), s1.cuda(), ssc.cuda()
    what = f'dis_dembed {(h, w, c, e, cimg)}'
    part = _twice(lambda: _window_sums(dc1d, c))
    _check_window_sums(part, dc1, what)

    def run():
        de = _nan((n, e))
        _ck(_lib().mcgen_cgan_dis_dembed(_p(part), _p(dyd), _p(w1d), _p(wscd), _p(s1d), _p(sscd), _p(de), _dt(dtype), n, h, c, cin, cimg,
                                         e, hwq, c + 8, _stream()), 'dis_dembed')
        return de
    got = _twice(run)
    ref, mag = R.dis_dembed(dc1, dy, torch.nan_to_num(w1), torch.nan_to_num(wsc), float(s1), float(ssc), cimg, e)
    g, s = 1024 // c, 1024 // e
    per = (10 * c + s - 1) // s
    chain = max(w + h + 9, (hwq + g - 1) // g + g) + 4 + per + s
    _assert_within(got, ref, 2 * chain * U32 * mag, what)
    _assert_bits(_ops().cgan_dis_dembed(dc1d, c, dyd, w1d, wscd, s1d, sscd, cimg, e), got, 'wrapper')


def test_cgan_dis_dembed_refuses_1032_channels():
    n, h, c, e = 1, 2, 1032, 1
    part, dy = torch.zeros(n, h, 3, c).cuda(), torch.zeros(n, 1, c).cuda()
    w1, wsc, one = torch.zeros(c, e, 3, 3).cuda(), torch.zeros(c, e).cuda(), torch.ones(1).cuda()
    de = _nan((n, e))
    rc = _lib().mcgen_cgan_dis_dembed(_p(part), _p(dy), _p(w1), _p(wsc), _p(one), _p(one), _p(de), _dt(torch.float32), n, h, c, e, 0, e,
                                      1, c, _stream())
    _refused(rc, 'cgan_dis_dembed: 1032 channels do not fit the LDS plan (at most 1024)')
    torch.cuda.synchronize()
    assert bool(torch.isnan(de).all())


ENC_MAPS = [(2, 2, 8, 1, 0), (2, 2, 8, 256, 1), (4, 6, 24, 32, 3), (6, 4, 960, 256, 1), (2, 2, 960, 32, 3), (4, 4, 24, 1, 1)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('ho,wo,c,e,cimg', ENC_MAPS)
def test_cvae_enc_dembed(ho, wo, c, e, cimg, dtype):
    """C = 960 asks for exactly 64 KB of dynamic LDS: the launch must be accepted (a refused launch raises here)."""
    gen = _gen(ho * wo + c + e + 1)
    n, cin = 2, cimg + e + 1
    d_h = _randn(gen, n, ho, wo, c, dtype=dtype)
    wc = torch.full((c, cin, 4, 4), NAN)
    wc[:, cimg:cimg + e] = torch.randn(c, e, 4, 4, generator=gen)
    dhd, wcd = _padded(d_h, c + 8, dtype), wc.cuda()
    what = f'enc_dembed {(ho, wo, c, e, cimg)}'
    part = _twice(lambda: _window_sums(dhd, c))
    _check_window_sums(part, d_h, what)

    def run():
        de = _nan((n, e))
        _ck(_lib().mcgen_cvae_enc_dembed(_p(part), _p(wcd), _p(de), n, ho, c, cin, cimg, e, _stream()), 'enc_dembed')
        return de
    got = _twice(run)
    ref, mag = R.enc_dembed(d_h, torch.nan_to_num(wc), cimg, e)
    s = 1024 // e
    per = (16 * c + s - 1) // s
    _assert_within(got, ref, 2 * (wo + ho + 9 + 1 + per + s) * U32 * mag, what)
    _assert_bits(_ops().cvae_enc_dembed(dhd, wcd, cimg, e), got, 'wrapper')


def test_cvae_enc_dembed_refuses_968_channels():
    n, h, c, e = 1, 2, 968, 1
    part, wc = torch.zeros(n, h, 3, c).cuda(), torch.zeros(c, e, 4, 4).cuda()
    de = _nan((n, e))
    rc = _lib().mcgen_cvae_enc_dembed(_p(part), _p(wc), _p(de), n, h, c, e, 0, e, _stream())
    _refused(rc, 'cvae_enc_dembed: 968 channels do not fit the LDS plan (at most 960)')
    torch.cuda.synchronize()
    assert bool(torch.isnan(de).all())


# ---- 5. the CVAE latent step ------------------------------------------------------------------------------------------------
LATENT = [(1, 1, 1), (16, 32, 10), (255, 256, 3), (257, 4, 5)]


def _latent_case(lat, e, m, dtype, gen, overflow):
    n = 5
    lab = _labels(gen, n, m)
    mu = _randn(gen, n, lat, dtype=dtype)
    lv = (torch.rand(n, lat, generator=gen) * 50 - 30).to(dtype)
    lv[1, 0], lv[2, -1] = -30.0, 20.0
    eps = torch.randn(n, lat, generator=gen)
    if overflow:
        lv[3, lat // 2] = 200.0
        eps[3, lat // 2] = -1.5
    return n, lab, mu, lv, eps, _poison_columns(torch.randn(e, m, generator=gen), lab)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('overflow', [False, True])
@pytest.mark.parametrize('lat,e,m', LATENT)
def test_cvae_latent_fwd(lat, e, m, overflow, dtype):
    gen = _gen(lat + e)
    n, lab, mu, lv, eps, w = _latent_case(lat, e, m, dtype, gen, overflow)
    ldm, cp = 2 * lat + 8, (lat + e + 7) // 8 * 8 + 8
    mld, wd, labd = _padded(torch.cat([mu, lv], 1), ldm, dtype), w.cuda(), lab.cuda()
    for use_eps in (True, False):
        epsd = eps.cuda() if use_eps else None

        def run():
            o_mu, o_lv, zrow, kl, kld = _nan((n, lat)), _nan((n, lat)), _nan((n, cp), dtype), _nan((n,)), _nan((1,))
            _ck(_lib().mcgen_cvae_latent_fwd(_p(mld), ldm, _p(epsd), _p(wd), _p(labd), _p(o_mu), _p(o_lv), _p(zrow), _p(kl), _p(kld),
                                             _dt(dtype), n, lat, e, m, cp, _stream()), 'latent_fwd')
            return o_mu, o_lv, zrow, kl, kld
        o_mu, o_lv, zrow, kl, kld = _twice(run)
        what = f'latent_fwd {(lat, e, m)} overflow={overflow} eps={use_eps}'
        f = R.latent_fwd(torch.cat([mu, lv], 1), eps if use_eps else None, w, lab)
        _assert_bits(o_mu, mu.float(), what + ': mu')
        _assert_bits(o_lv, lv.float(), what + ': logvar')
        ref_tail = torch.zeros(n, cp - lat, dtype=F64)
        ref_tail[:, :e] = f['zrow'][:, lat:]
        _assert_bits(zrow[:, lat:].contiguous(), ref_tail.to(dtype), what + ': embedding and pad')
        z, zg = f['z'].clone(), zrow[:, :lat].double().cpu()
        finite = torch.ones(n, lat, dtype=torch.bool)
        if overflow and use_eps:
            finite[3, lat // 2] = False                                        # expf(100) overflows fp32: z = mu + eps * inf
            assert float(zg[3, lat // 2]) == -INF, what
            z[3, lat // 2] = zg[3, lat // 2] = 0.0
        if use_eps:
            t32 = 2 * (3 * U32 * torch.where(finite, f['noise'], torch.zeros_like(z)).abs() + U32 * z.abs())
            _assert_within(zg, z, _out_tol(z, t32, dtype), what + ': z')
        else:
            _assert_bits(zrow[:, :lat].contiguous(), mu, what + ': z = mu')
        klg = kl.double().cpu()
        if overflow:
            assert float(klg[3]) == INF and float(f['kl'][3]) > 3e38, what + ': kl of the overflowing sample'
            assert float(kld) == INF, what + ': kld'
        rows = [i for i in range(n) if not (overflow and i == 3)]
        assert bool(torch.isfinite(klg[rows]).all()), what + ': the other samples stay finite'
        tol = 2 * (4 * math.ceil(lat / 256) + 10) * U32 * f['kl_mag']
        _assert_within(klg[rows], f['kl'][rows], tol[rows], what + ': kl')
        if not overflow:
            _assert_within(kld, klg.sum().reshape(1), 2 * n * U32 * klg.abs().sum().reshape(1), what + ': kld from the kernel\'s kl')
    if not overflow:
        wr = _ops().cvae_latent_fwd(mld, eps.cuda(), wd, labd, lat)
        ref = _twice(lambda: _run_latent_wrapper_shape(mld, ldm, eps.cuda(), wd, labd, n, lat, e, m, dtype))
        _assert_bits(wr[2].reshape(n, -1), ref[0], 'wrapper zrow')
        _assert_bits(wr[3], ref[1], 'wrapper kld')


def _run_latent_wrapper_shape(mld, ldm, epsd, wd, labd, n, lat, e, m, dtype):
    cp = (lat + e + 7) // 8 * 8
    o_mu, o_lv, zrow, kl, kld = _nan((n, lat)), _nan((n, lat)), _nan((n, cp), dtype), _nan((n,)), _nan((1,))
    _ck(_lib().mcgen_cvae_latent_fwd(_p(mld), ldm, _p(epsd), _p(wd), _p(labd), _p(o_mu), _p(o_lv), _p(zrow), _p(kl), _p(kld),
                                     _dt(dtype), n, lat, e, m, cp, _stream()), 'latent_fwd')
    return zrow, kld


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('lat,e,m', LATENT + [(16, 0, 1)])
def test_cvae_latent_bwd(lat, e, m, dtype):
    gen = _gen(lat + e + 1)
    n, _, mu, lv, eps, _ = _latent_case(lat, max(e, 1), m, torch.float32, gen, False)
    dz, dcols = _randn(gen, n, lat, dtype=dtype), _randn(gen, n, e, dtype=dtype)
    ldz, cq = lat + e + 8, (2 * lat + 7) // 8 * 8 + 8
    inv = PR.f32(1.0 / 3072)
    dzd = _padded(torch.cat([dz, dcols], 1), ldz, dtype)
    mud, lvd, epsd = mu.cuda(), lv.cuda(), eps.cuda()

    def run():
        dml, de = _nan((n, cq), dtype), (_nan((n, e)) if e else None)
        _ck(_lib().mcgen_cvae_latent_bwd(_p(dzd), ldz, _p(mud), _p(lvd), _p(epsd), inv, _p(dml), _p(de), _dt(dtype), n, lat, e, cq,
                                         _stream()), 'latent_bwd')
        return dml, de
    dml, de = _twice(run)
    what = f'latent_bwd {(lat, e, m)}'
    b = R.latent_bwd(dz, mu, lv, eps, inv)
    if e:
        _assert_bits(de, dcols.float(), what + ': de')
    assert bool((dml[:, 2 * lat:] == 0).all()), what + ': pad'
    t_mu = 2 * (U32 * b['dmu_terms'][1].abs() + U32 * b['dmu'].abs())
    _assert_within(dml[:, :lat], b['dmu'], _out_tol(b['dmu'], t_mu, dtype), what + ': dmu')
    ta, tb = b['dlogvar_terms']
    t_lv = 2 * (4 * U32 * ta.abs() + (2 * U32 * b['exp_lv'] + U32 * (b['exp_lv'] - 1).abs()) * 0.5 * inv + U32 * tb.abs()
                + U32 * b['dlogvar'].abs())
    _assert_within(dml[:, lat:2 * lat], b['dlogvar'], _out_tol(b['dlogvar'], t_lv, dtype), what + ': dlogvar')
    wr = _ops().cvae_latent_bwd(dzd, mud, lvd, epsd, inv, e) if e else None
    if wr is not None:
        _assert_bits(wr[0].reshape(n, -1), dml[:, :wr[0].shape[-1]].contiguous(), 'wrapper dml')
        _assert_bits(wr[1], de, 'wrapper de')


# ---- 6. the CGlow prior -------------------------------------------------------------------------------------------------------
PRIOR = [(1, 1, 2, 1, 0), (1025, 1, 258, 3, 20001), (3, 6, 520, 10, 7), (1025, 3, 8, 1623, 0)]


def _prior_case(n, c2, m, gen):
    lab = _labels(gen, n, m)
    b_p, b_e = torch.randn(c2, generator=gen), torch.randn(c2, generator=gen)
    s_p, s_e = torch.rand(c2, generator=gen) * 6 - 3, torch.rand(c2, generator=gen) * 6 - 3
    s_p[0], s_e[0], s_p[-1], s_e[-1] = 3.0, -3.0, -3.0, 3.0
    w_e = _poison_columns(torch.randn(c2, m, generator=gen), lab)
    return lab, b_p, s_p, w_e, b_e, s_e


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,hw,c2,m,dwp', PRIOR)
def test_cglow_prior(n, hw, c2, m, dwp, dtype):
    gen = _gen(n + c2)
    lab, b_p, s_p, w_e, b_e, s_e = _prior_case(n, c2, m, gen)
    cp = (c2 + 7) // 8 * 8 + 8
    dev = [t.cuda() for t in (b_p, s_p, w_e, b_e, s_e, lab)]

    def run():
        out = _nan((n, hw, cp), dtype)
        _ck(_lib().mcgen_cglow_prior(*[_p(t) for t in dev], _p(out), _dt(dtype), n, hw, c2, m, cp, _stream()), 'cglow_prior')
        return out
    got = _twice(run)
    ref, (t1, t2) = R.prior(b_p, s_p, torch.nan_to_num(w_e), b_e, s_e, lab, hw)
    what = f'cglow_prior {(n, hw, c2, m)}'
    assert bool((got[..., c2:] == 0).all()), what + ': pad'
    if hw > 1:
        _assert_bits(got[:, 1:].contiguous(), got[:, :1].expand(-1, hw - 1, -1).contiguous(), what + ': every pixel the same')
    t32 = 2 * ((3 * s_p.abs().double() + 4) * U32 * t1 + (3 * s_e.abs().double() + 5) * U32 * t2 + U32 * ref[:, 0].abs())
    _assert_within(got[..., :c2], ref, _out_tol(ref, t32[:, None, :], dtype), what)
    wr = _ops().cglow_prior(*dev, hw, 1, dtype)
    _assert_bits(wr.reshape(n, hw, -1), got[..., :wr.shape[-1]].contiguous(), 'wrapper')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,hw,c2,m,dwp', PRIOR)
def test_cglow_prior_bwd(n, hw, c2, m, dwp, dtype):
    gen = _gen(n + c2 + 1)
    lab, b_p, s_p, w_e, b_e, s_e = _prior_case(n, c2, m, gen)
    cp = (c2 + 7) // 8 * 8 + 8
    dprior = _randn(gen, n, hw, c2, dtype=dtype)
    dpd = _padded(dprior, cp, dtype)
    dev = [t.cuda() for t in (b_p, s_p, w_e, b_e, s_e, lab)]
    if dwp > 64 * 256:
        assert dwp % 256                                                           # the zero fill's stride loop, ragged

    def run():
        ws = _nan((2, n, c2))
        db_p, ds_p, db_e, ds_e, dw_e = _nan((c2,)), _nan((c2,)), _nan((c2,)), _nan((c2,)), _nan((c2, m))
        dw_p = _nan((dwp,)) if dwp else None
        _ck(_lib().mcgen_cglow_prior_bwd(_p(dpd), *[_p(t) for t in dev], _p(ws), _p(db_p), _p(ds_p), _p(dw_p), dwp, _p(dw_e), _p(db_e),
                                         _p(ds_e), _dt(dtype), n, hw, c2, m, cp, _stream()), 'cglow_prior_bwd')
        return ws, db_p, ds_p, db_e, ds_e, dw_e, dw_p
    ws, db_p, ds_p, db_e, ds_e, dw_e, dw_p = _twice(run)
    what = f'cglow_prior_bwd {(n, hw, c2, m, dwp)}'
    if dwp:
        assert bool((dw_p == 0).all()), what + ': dw_p'
    clean = torch.nan_to_num(w_e)
    g0, m0 = R.prior_bwd(dprior, b_p, s_p, clean, b_e, s_e, lab)
    dh, de = ws[0].cpu(), ws[1].cpu()
    if hw == 1:
        _assert_bits(dh, dprior[:, 0].float(), what + ': dh of one pixel')
    t_dh = 2 * hw * U32 * m0['dh']
    _assert_within(dh, g0['dh'], t_dh, what + ': dh')
    re, ke = torch.exp(3 * s_e.double()), (3 * s_e.abs().double() + 4) * U32
    _assert_within(de, g0['dh'] * re, (t_dh + 2 * ke * g0['dh'].abs()) * re, what + ': de')
    # the parameter gradients from the dh the kernel wrote (chains of N), the table gradient from its own rows
    g, mg = R.prior_bwd(dh[:, None, :], b_p, s_p, clean, b_e, s_e, lab)
    for key, got, s in (('b_p', db_p, s_p), ('s_p', ds_p, s_p), ('b_e', db_e, s_e), ('s_e', ds_e, s_e)):
        _assert_within(got, g[key], 2 * (n + 3 * s.abs().double() + 8) * U32 * mg[key], f'{what}: d{key}')
    ref_w, mag_w = R.embed_bwd(de, lab, m)
    _assert_within(dw_e, ref_w, _embed_bwd_tol(lab, m, mag_w, False), what + ': dw_e')
    _assert_within(dw_e, g0['w_e'], _embed_bwd_tol(lab, m, m0['w_e'], False) + 2 * (hw + 3 * s_e.abs().double()[:, None] + 4) * U32 * m0['w_e'],
                   what + ': dw_e end to end')
    outs = [_nan((c2,)) for _ in range(4)] + [_nan((c2, m))]
    wp = _nan((dwp,)) if dwp else None
    _ops().cglow_prior_bwd(dpd, *dev, outs[0], outs[1], wp, outs[4], outs[2], outs[3])
    for a, b in zip(outs, (db_p, ds_p, db_e, ds_e, dw_e)):
        _assert_bits(a, b, 'wrapper')


# ---- 7. the conditional gates of CPixelCNN -----------------------------------------------------------------------------------
# 105 pixels: 6 blocks of 18, the last holds 15; 322 pixels: 20 blocks of 17, block 18 holds 16 and block 19 none
GATE_PIXELS = [(3, 35), (7, 46)]
GATE_M = 5


def _stats_blocks(pixels):
    """ops.cpx_gated_bwd / ops.cpx_gate_stats: one block per 16 pixels, 256 at most."""
    return max(1, min(256, pixels // 16))


def _gate_case(n, hw, c, dtype, gen):
    """s [N, HW, 2C], table [M, 2C] (NaN in the rows no clamped label reads), labels with -1 and M + 3, scale, shift.
    Channel 0: s + e = 0.5 exactly at every third pixel with scale 2, shift -1 (z = 0 exactly); the last two channels of the
    second half have e_b = +100 and -100."""
    lab = torch.randint(0, GATE_M, (n,), generator=gen)
    lab[0] = -1
    lab[-1] = GATE_M + 3
    if n > 2:
        lab[1] = 2
    s = _randn(gen, n, hw, 2 * c, dtype=dtype)
    s[..., c:] *= 3
    table = torch.randn(GATE_M, 2 * c, generator=gen)
    table[:, 0] = 0.25
    s[:, ::3, 0] = 0.25
    table[:, 2 * c - 2], table[:, 2 * c - 1] = 100.0, -100.0
    absent = torch.ones(GATE_M, dtype=torch.bool)
    absent[lab.clamp(0, GATE_M - 1)] = False
    table[absent] = NAN
    sc, sh = _vec(gen, c), _vec(gen, c, 0.5)
    sc[0], sh[0] = 2.0, -1.0
    return s, table, lab, sc, sh


def _gate_errs(s, table, lab, sc, sh):
    """The fp32 gate quantities and their error bounds (float64): x = s + e is one rounding (u |x|); z = fma(x, scale,
    shift): dz_ = |scale| u |x| + u |z|; q = sigmoid(bb), bb = b + e_b rounded once: dq = 5u q + u |bb| q (1 - q)."""
    c = sc.numel()
    x = R.cpx_gate_input(s, torch.nan_to_num(table), lab)
    a, bb = x[..., :c], x[..., c:]
    z = a * sc.double() + sh.double()
    q = torch.sigmoid(bb)
    ez = sc.double().abs() * U32 * a.abs() + U32 * z.abs()
    eq = 5 * U32 * q + U32 * bb.abs() * q * (1 - q)
    near = (z != 0) & (z.abs() <= 2 * ez)                                      # the computed sign of z may differ from the exact one
    return dict(a=a, bb=bb, z=z, q=q, ez=ez, eq=eq, near=near)


def _cgate(items, fwd, blocks=None, rows=None):
    """mcgen_cgate_t jobs from (s [N, HW, 2C], table, label[, scale, shift]) device tensors -> (array, outputs).  Statistics:
    job i gets blocks[i] blocks and a NaN partials buffer of rows[i] >= blocks[i] rows."""
    from mcgen_amd import _lib as L
    arr = (L.CGate * len(items))()
    outs = []
    for i, (d, it) in enumerate(zip(arr, items)):
        s, table, lab = it[:3]
        n, hw, c2 = s.shape
        d.s, d.table, d.label = _p(s), _p(table), _p(lab)
        d.N, d.HW, d.C, d.M = n, hw, c2 // 2, table.shape[0]
        if fwd:
            out = _nan((n, hw, c2 // 2), s.dtype)
            d.scale, d.shift, d.out = _p(it[3]), _p(it[4]), _p(out)
        else:
            out = _nan((rows[i] if rows else blocks[i], 2, c2 // 2))
            d.partials, d.blocks = _p(out), blocks[i]
        outs.append(out)
    return arr, outs


def _gate_stats(items, blocks, rows=None):
    arr, outs = _cgate(items, False, blocks, rows)
    _ck(_lib().mcgen_cpx_gate_stats(arr, len(items), _dt(items[0][0].dtype), _stream()), 'cpx_gate_stats')
    torch.cuda.synchronize()
    return tuple(outs)


def _gate_fwd(items):
    arr, outs = _cgate(items, True)
    _ck(_lib().mcgen_cpx_gated_fwd(arr, len(items), _dt(items[0][0].dtype), _stream()), 'cpx_gated_fwd')
    torch.cuda.synchronize()
    return tuple(outs)


def _block_sums(terms, errs, pixels, blocks, lanes):
    """Per-block sums of per-pixel terms [pixels, C] and their bound: each term within errs, a lane adds ceil(ppb / lanes)
    terms and the block its lanes, in fp32; doubled.  -> (ref [blocks, C], tol [blocks, C], ppb)."""
    ppb = (pixels + blocks - 1) // blocks
    chain = (ppb + lanes - 1) // lanes + lanes
    ref, tol = torch.zeros(blocks, terms.shape[1], dtype=F64), torch.zeros(blocks, terms.shape[1], dtype=F64)
    for b in range(blocks):
        t, e = terms[b * ppb:(b + 1) * ppb], errs[b * ppb:(b + 1) * ppb]
        ref[b], tol[b] = t.sum(0), 2 * (e.sum(0) + chain * U32 * t.abs().sum(0))
    return ref, tol, ppb


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,hw', GATE_PIXELS)
@pytest.mark.parametrize('c', [8, 2048])
def test_cpx_gate_stats(c, n, hw, dtype):
    """partials[b] = (sum x, sum x^2) of x = a + e_a over block b's pixels: the terms are within u |x| and 3u x^2."""
    gen = _gen(c + n)
    s, table, lab, sc, sh = _gate_case(n, hw, c, dtype, gen)
    pixels, blocks = n * hw, _stats_blocks(n * hw)
    item = (s.cuda(), table.cuda(), lab.cuda())
    part, = _twice(lambda: _gate_stats([item], [blocks]))
    ppb = _check_partials(part, pixels, blocks, 'cpx_gate_stats')
    assert pixels % ppb and hw % ppb                                            # a ragged block, blocks that straddle images
    a = _gate_errs(s, table, lab, sc, sh)['a'].reshape(pixels, c)
    lanes = 256 // (c // 8)
    r1, t1, _ = _block_sums(a, U32 * a.abs(), pixels, blocks, lanes)
    r2, t2, _ = _block_sums(a * a, 3 * U32 * a * a, pixels, blocks, lanes)
    _assert_within(part[:, 0], r1, t1, f'sum C={c} {(n, hw)}')
    _assert_within(part[:, 1], r2, t2, f'sum of squares C={c} {(n, hw)}')
    wr, = _ops().cpx_gate_stats([(item[0].view(n, 1, hw, 2 * c), item[1], item[2])])
    _assert_bits(wr, part, 'wrapper')


def _gated_fwd_tol(g, ref, dtype):
    """out = relu(z) / (1 + expf(-bb)): |d out| <= dz_ q + relu(z) dq + u |out|, doubled, with the flush floor."""
    rz = g['z'].clamp_min(0)
    return _out_tol(ref, 2 * (g['ez'] * g['q'] + rz * g['eq'] + U32 * ref.abs()) + TINY * rz.clamp_min(1), dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,hw', GATE_PIXELS)
@pytest.mark.parametrize('c', [8, 24, 2048])
def test_cpx_gated_fwd(c, n, hw, dtype):
    gen = _gen(c + n + 1)
    s, table, lab, sc, sh = _gate_case(n, hw, c, dtype, gen)
    item = tuple(t.cuda() for t in (s, table, lab, sc, sh))
    got, = _twice(lambda: _gate_fwd([item]))
    g = _gate_errs(s, table, lab, sc, sh)
    ref = R.cpx_gated_fwd(s, torch.nan_to_num(table), lab, sc, sh)
    assert bool((g['z'] == 0).any()) and bool((g['z'] > 0).any()) and bool((g['z'] < 0).any())
    _assert_within(got, ref, _gated_fwd_tol(g, ref, dtype), f'cpx_gated_fwd C={c} {(n, hw)}')
    assert bool((got[:, ::3, 0] == 0).all())                                    # z = 0 exactly
    wr, = _ops().cpx_gated_fwd([(item[0].view(n, 1, hw, 2 * c),) + item[1:]])
    _assert_bits(wr, got, 'wrapper')


def test_cpx_statistics_refuse_24_channels():
    gen = _gen(24)
    n, hw, c = 2, 8, 24
    s, table, lab, sc, sh = _gate_case(n, hw, c, torch.float32, gen)
    item = (s.cuda(), torch.nan_to_num(table).cuda(), lab.cuda())
    arr, (part,) = _cgate([item], False, [1])
    _refused(_lib().mcgen_cpx_gate_stats(arr, 1, _dt(torch.float32), _stream()), 'cpx_gate_stats: job 0 needs partials, blocks > 0 and C/8 dividing 256')
    ds = _nan(s.shape)
    v = _nan((c,))
    rc = _lib().mcgen_cpx_gated_bwd_stats(_p(item[0]), _p(item[1]), _p(item[2]), GATE_M, _p(v), _p(v), _p(v), _p(v), _p(ds), _p(ds),
                                          _p(part), 1, _dt(torch.float32), n, hw, c, _stream())
    _refused(rc, 'cpx_gated_bwd_stats: C/8 must divide 256')
    torch.cuda.synchronize()
    assert bool(torch.isnan(part).all()) and bool(torch.isnan(ds).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_cpx_gate_jobs_of_unequal_size(dtype):
    """One launch of three jobs with different N, HW, C and blocks (the grid is sized by the largest): each job's output
    equals that of a launch of that job alone, bit for bit, in both orders; the partials of a job with fewer blocks have
    NaN rows up to the largest job's count, which the launch must leave alone."""
    gen = _gen(7)
    dims = [(3, 35, 8, 6), (1, 7, 64, 1), (7, 46, 2048, 20)]                   # (N, HW, C, blocks)
    cases = [[t.cuda() for t in _gate_case(n, hw, c, dtype, gen)] for n, hw, c, _ in dims]
    blocks = [b for *_, b in dims]
    single_p = [_gate_stats([k[:3]], [b])[0] for k, b in zip(cases, blocks)]
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        parts = _twice(lambda: _gate_stats([cases[i][:3] for i in order], [blocks[i] for i in order], [max(blocks)] * 3))
        for i, part in zip(order, parts):
            _assert_bits(part[:blocks[i]].contiguous(), single_p[i], f'statistics {order}, job {i}')
            assert bool(torch.isnan(part[blocks[i]:]).all()), f'statistics {order}, job {i}: rows past its blocks were written'
    fdims = [(3, 35, 24), (1, 7, 8), (2, 16, 2048)]
    fcases = [tuple(t.cuda() for t in _gate_case(n, hw, c, dtype, gen)) for n, hw, c in fdims]
    single_f = [_gate_fwd([k])[0] for k in fcases]
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        outs = _twice(lambda: _gate_fwd([fcases[i] for i in order]))
        for i, out in zip(order, outs):
            _assert_bits(out, single_f[i], f'forward {order}, job {i}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n,hw', GATE_PIXELS)
@pytest.mark.parametrize('c', [8, 2048])
def test_cpx_gated_bwd(c, n, hw, dtype):
    """Pass 1 with the wrapper's block rule.  dz = g q [z > 0]: |g| dq + u |dz|, either value where the sign of z is in doubt.
    db = g relu(z) q (1 - q): |g| (dz_ q (1 - q) + relu(z) (dq (1 - q) + q (dq + u (1 - q)))) + 4u |db|.  Per-block partials of
    dz and dz xhat, xhat = (x - mean) rstd within (u |x| + u |x - mean|) rstd + u |xhat|, by _block_sums; all doubled, with
    the flush floor.  Pass 2 reads back the stored dz and the fp32 sums: da = scale (dz - (S1 + xhat S2) inv) is within
    |scale| (2u T1 + 5u T2 + 8u T3 + u |x| rstd |S2 inv|) + u |da| (test_pixel_vq_kernels_gpu._apply_tol plus the rounding of
    x), doubled; the db half keeps its bits.  dsum: the first half sums the unrounded da (HW terms), the second half the
    stored db."""
    ops, lib = _ops(), _lib()
    gen = _gen(c + n + 2)
    s, table, lab, sc, sh = _gate_case(n, hw, c, dtype, gen)
    gr = _randn(gen, n, hw, c, dtype=dtype)
    mean, rstd = _vec(gen, c, 0.5), torch.rand(c, generator=gen) + 0.5
    pixels, blocks, lanes = n * hw, _stats_blocks(n * hw), 256 // (c // 8)
    sd, td, ld, scd, shd, md, rd, gd = (t.cuda() for t in (s, table, lab, sc, sh, mean, rstd, gr))

    def pass1():
        ds, part = _nan(s.shape, dtype), _nan((blocks, 2, c))
        _ck(lib.mcgen_cpx_gated_bwd_stats(_p(sd), _p(td), _p(ld), GATE_M, _p(scd), _p(shd), _p(md), _p(rd), _p(gd), _p(ds), _p(part), blocks,
                                          _dt(dtype), n, hw, c, _stream()), 'cpx_gated_bwd_stats')
        return ds, part
    ds, part = _twice(pass1)
    _check_partials(part, pixels, blocks, 'cpx_gated_bwd_stats')
    e = _gate_errs(s, table, lab, sc, sh)
    clean = torch.nan_to_num(table)
    dz, db, _, _ = R.cpx_gated_bwd_stats(s, clean, lab, sc, sh, mean, rstd, gr)
    g64, q, rz = gr.double().abs(), e['q'], e['z'].clamp_min(0)
    e_dz = g64 * e['eq'] + U32 * dz.abs()
    e_dz = torch.where(e['near'], e_dz + g64 * q, e_dz)
    e_db = g64 * (e['ez'] * q * (1 - q) + rz * (e['eq'] * (1 - q) + q * (e['eq'] + U32 * (1 - q)))) + 4 * U32 * db.abs()
    floor = TINY * g64 * rz.clamp_min(1)
    _assert_within(ds[..., :c], dz, _out_tol(dz, 2 * e_dz + floor, dtype), 'dz')
    _assert_within(ds[..., c:], db, _out_tol(db, 2 * e_db + floor, dtype), 'db')
    assert bool((ds[:, ::3, 0] == 0).all())                                     # z = 0 exactly: the ReLU's gradient is 0
    xm = e['a'] - mean.double()
    xh = xm * rstd.double()
    e_xh = (U32 * e['a'].abs() + U32 * xm.abs()) * rstd.double() + U32 * xh.abs()
    t2 = dz * xh
    r1, tol1, _ = _block_sums(dz.reshape(pixels, c), (e_dz + floor).reshape(pixels, c), pixels, blocks, lanes)
    r2, tol2, _ = _block_sums(t2.reshape(pixels, c), ((e_dz + floor) * xh.abs() + dz.abs() * e_xh + U32 * t2.abs()).reshape(pixels, c),
                              pixels, blocks, lanes)
    _assert_within(part[:, 0], r1, tol1, 'partials of dz')
    _assert_within(part[:, 1], r2, tol2, 'partials of dz xhat')
    dgamma, dbeta = _nan((c,)), _nan((c,))
    sums = ops._bwd_sums(part, c, dgamma, dbeta)
    stored = ds.clone()

    def pass2():
        d2, dsum = stored.clone(), _nan((n, 2 * c))
        _ck(lib.mcgen_cpx_gated_bwd_apply(_p(d2), _p(sd), _p(td), _p(ld), GATE_M, _p(sums), _p(scd), _p(md), _p(rd), float(pixels), _p(dsum),
                                          _dt(dtype), n, hw, c, _stream()), 'cpx_gated_bwd_apply')
        return d2, dsum
    d2, dsum = _twice(pass2)
    inv = PR.f32(1.0 / pixels)
    dz_read, sm = stored[..., :c].cpu().double(), sums.cpu().double()
    ref = PR.bn_apply(dz_read, e['a'], sc, mean, rstd, sm[0], sm[1], 1.0 / inv)
    k = sc.double().abs()
    t32 = 2 * (k * (2 * U32 * dz_read.abs() + 5 * U32 * (sm[0] * inv).abs() + 8 * U32 * (xh * sm[1] * inv).abs()
                    + U32 * e['a'].abs() * rstd.double() * (sm[1] * inv).abs()) + U32 * ref.abs())
    _assert_within(d2[..., :c], ref, _out_tol(ref, t32, dtype), 'da')
    _assert_bits(d2[..., c:].contiguous(), stored[..., c:].contiguous(), 'db after the apply pass')
    _assert_within(dsum[:, :c], ref.sum(1), t32.sum(1) + 2 * hw * U32 * ref.abs().sum(1), 'dsum of da')
    dbs = stored[..., c:].cpu().double()
    _assert_within(dsum[:, c:], dbs.sum(1), 2 * hw * U32 * dbs.abs().sum(1), 'dsum of db')
    dg2, db2 = _nan((c,)), _nan((c,))
    wds, wsum = ops.cpx_gated_bwd(sd.view(n, 1, hw, 2 * c), td, ld, scd, shd, md, rd, gd.view(n, 1, hw, c), dg2, db2)
    _assert_bits(wds, d2, 'wrapper ds')
    _assert_bits(wsum, dsum, 'wrapper dsum')
    assert torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)


# ---- 8. the table gradient and the sampler's row gather ------------------------------------------------------------------
@pytest.mark.parametrize('n,c2,m', [(5, 16, 1), (1, 16, 5), (5, 656, 1623)])
def test_cpx_embed_bwd(n, c2, m):
    gen = _gen(n + c2)
    if m * c2 > 16 * 5:
        assert m * c2 > GRID_ITEMS and (m * c2) % 256                              # a ragged second grid pass
    lab = torch.randint(0, m, (n,), generator=gen)
    if n > 1:
        lab[0], lab[1], lab[-1] = -1, m, lab[2]
    dv, dh = torch.randn(n, c2, generator=gen), torch.randn(n, c2, generator=gen)
    dvd, dhd, labd = dv.cuda(), dh.cuda(), lab.cuda()
    cnt = torch.bincount(lab[_inside(lab, m)], minlength=m).double()[:, None]
    for two in (False, True):
        def run():
            de = _nan((m, c2))
            _ck(_lib().mcgen_cpx_embed_bwd(_p(dvd) if two else None, _p(dhd), _p(labd), _p(de), n, c2, m, _stream()), 'cpx_embed_bwd')
            return de
        got = _twice(run)
        ref, mag = R.cpx_embed_bwd(dv if two else None, dh, lab, m)
        _assert_within(got, ref, 2 * 2 * cnt * U32 * mag, f'cpx_embed_bwd {(n, c2, m)} two={two}')
        assert bool((got.cpu()[cnt[:, 0] == 0] == 0).all())
    de = _nan((m, c2))
    _ops().cpx_embed_bwd(dvd, dhd, labd, de)
    _assert_bits(de, got, 'wrapper')


@pytest.mark.parametrize('nl,n,c2,m', [(2, 5, 16, 1), (3, 1, 16, 5), (15, 37, 2048, 7)])
def test_cpx_gather_rows(nl, n, c2, m):
    gen = _gen(nl + n)
    if nl == 15:
        assert nl * n * c2 > GRID_ITEMS
    lab = torch.randint(0, m, (n,), generator=gen)
    if n > 1:
        lab[0], lab[1] = -1, m + 2
    tables = torch.randn(nl, m, c2, generator=gen)
    absent = torch.ones(m, dtype=torch.bool)
    absent[lab.clamp(0, m - 1)] = False
    tables[:, absent] = NAN
    td, labd = tables.cuda(), lab.cuda()

    def run():
        out = _nan((nl, n, c2))
        _ck(_lib().mcgen_cpx_gather_rows(_p(td), _p(labd), _p(out), nl, n, c2, m, _stream()), 'cpx_gather_rows')
        return out
    got = _twice(run)
    _assert_bits(got, R.cpx_gather_rows(tables, lab).float(), f'cpx_gather_rows {(nl, n, c2, m)}')
    _assert_bits(_ops().cpx_gather_rows(td, labd), got, 'wrapper')


# ---- 9. the code embedding's gradient ---------------------------------------------------------------------------------------
def _codes(p, k, gen):
    codes = torch.randint(0, k, (p,), generator=gen)
    if p >= 256 and k >= 3:
        codes[:256] = 1                                                        # a full LDS list for code 1, no match for the others
        codes[256:] = torch.where(codes[256:] == 1, torch.zeros_like(codes[256:]), codes[256:])
        if p > 512:
            codes[300], codes[301], codes[302] = -1, k, 10 ** 9
            codes[512:] = 1                                                    # code 1: full, empty, one match
    elif p > 8:
        codes[p - 3], codes[p - 5], codes[p - 7] = -1, k, 10 ** 9
    return codes


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('p,c,k', [(1, 1, 1), (255, 40, 4), (257, 256, 3), (513, 40, 3), (257, 1, 1)])
def test_cpx_code_embed_bwd(p, c, k, dtype):
    gen = _gen(p + c)
    codes = _codes(p, k, gen)
    dx = _randn(gen, p, c, dtype=dtype)
    room = (p + 255) // 256 * 256 + 256
    codes_buf = torch.full((room,), int(codes[p - 1].clamp(0, k - 1)))       # past P: a code that would match
    codes_buf[:p] = codes
    dx_buf = torch.full((room, c + 8), NAN, dtype=dtype)
    dx_buf[:p, :c] = dx
    cd, dxd = codes_buf.cuda(), dx_buf.cuda()

    def run():
        de = _nan((k, c))
        _ck(_lib().mcgen_cpx_code_embed_bwd(_p(dxd), c + 8, _p(cd), _p(de), p, k, c, _dt(dtype), _stream()), 'cpx_code_embed_bwd')
        return de
    got = _twice(run)
    ref, mag = R.cpx_code_embed_bwd(dx, codes, k)
    cnt = torch.bincount(codes[(codes >= 0) & (codes < k)], minlength=k).double()[:, None]
    _assert_within(got, ref, 2 * cnt * U32 * mag, f'cpx_code_embed_bwd {(p, c, k)}')
    if p == 257 and k == 3:
        assert int(cnt[1]) == 256 and int((codes[256:] == 1).sum()) == 0       # a full list, then a chunk without a match
    de = _nan((k, c))
    _ops().cpx_code_embed_bwd(dxd[:p].view(1, 1, p, c + 8), cd[:p].view(1, 1, p), de)
    _assert_bits(de, got, 'wrapper')


# ---- 10. the conditional sampler at full width ---------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.fixture(scope='module')
def full_model():
    """configs[4] of the conditional model: hidden 128, 15 layers, 512 codes, 1623 modes, seeded weights and perturbed
    BatchNorm statistics (as _full() of test_pixelcnn_sample_gpu.py)."""
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    from test_pixelcnn_sample_gpu import _perturb_bn
    cfg.update(model_name='cpixelcnn', device='cuda', classes_size=1623, compute_dtype='float32')
    cfg['pixelcnn'] = {'num_layer': 15, 'hidden_size': 128, 'num_embedding': 512}
    torch.manual_seed(4)
    m = models.cpixelcnn()
    return _perturb_bn(m, 5).cuda().train(False)


@pytest.mark.parametrize('h,w', [(8, 8), (4, 8)])
def test_conditional_sampler_full_width(full_model, h, w):
    """N = 37 (a ragged sample tile), labels with the first and the last of 1623 modes: the sampler's logits at every
    position against one eval forward on the drawn map, 1e-5 in fp32, 2e-2 for bf16 against the bf16 forward and 5e-2
    against the fp32 forward (the bounds of test_pixelcnn_sample_gpu.py)."""
    m, n = full_model, 37
    lab = torch.randint(0, 1623, (n,), generator=_gen(h)).cuda()
    lab[0], lab[-1] = 0, 1622

    def forward(codes, dtype):
        m.set_compute_dtype(dtype)
        with torch.no_grad():
            return m({'img': codes, 'label': lab})['logits']
    torch.manual_seed(h + w)
    m.set_compute_dtype(torch.float32)
    x = torch.zeros((n, h, w), dtype=torch.long, device='cuda')
    out, lg = m.sample(lab, x=x, return_logits=True)
    assert out is x and lg.shape == (n, 512, h, w) and int(out.min()) >= 0 and int(out.max()) < 512
    e32 = _rel(lg, forward(out, torch.float32))
    m.set_compute_dtype(torch.bfloat16)
    outb, lgb = m.sample(lab, x=torch.zeros_like(x), return_logits=True)
    b16, b32 = _rel(lgb, forward(outb, torch.bfloat16)), _rel(lgb, forward(outb, torch.float32))
    m.set_compute_dtype(torch.float32)
    print(f'\n[measured] conditional sampler {h}x{w}: fp32 {e32:.3g}, bf16 vs bf16 {b16:.3g}, bf16 vs fp32 {b32:.3g}')
    assert e32 <= 1e-5, e32
    assert b16 <= 2e-2 and b32 <= 5e-2, (b16, b32)
