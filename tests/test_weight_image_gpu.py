"""The weight-image builders of csrc/small_ops.hip one at a time -- prep_weight_kernel (ops.prep_weight, prep_weight_rows),
prep_weight_ex_body (ops.prep_weight_ex, prep_weight_ex_many), prep_weight_k_kernel (ops.prep_weight_k), the LDS-staged
batched prep_weight_body (ops.PrepBatch, ops.prep_and_codes) -- and the NCHW / NHWC converters, against
tests/weight_image_ref.py in float64.

All of these move data and apply a few fp32 operations per element, so nothing here has a fitted tolerance:

- exact inputs: weights are randn rounded to bf16 (8 significant bits), every scale (wscale, sigma, row / column scales)
  is a power of two in [1/4, 4].  wscale / sigma and every product are then exact in fp32 AND in bf16: the image must equal
  the float64 reference bit for bit, in both dtypes.
- rounded inputs: unrounded randn weights, sigma = 1.7, arbitrary scales.  With u = 2^-24, a correctly rounded fp32
  multiplication has relative error <= u and the device division <= 1 ulp <= 2u.  Per element, to first order:
      prep_weight / PrepBatch / prep_weight_k:  sc = wscale / sigma (2u), w * sc (u)                       -> 3u
      prep_weight_rows:                         w * 1 (exact), * row_scale[co] (u)                         ->  u
      prep_weight_ex:                           w * wscale (u), * row_scale[co] (u), * col_scale[ci] (u)   -> 3u
  All are within the 5u = 5 * 2^-24 * |ref| every fp32 image is held to (FP32_ULPS; one division and at most three
  multiplications).  The bf16 image must equal fp32_image.to(torch.bfloat16) bit for bit: one round-to-nearest-even of the
  same fp32 value.

Output buffers the caller owns start as NaN, so padding has to be WRITTEN as zero.  Where a wrapper allocates its own
output, a NaN-filled block of the same size is released to torch's caching allocator just before the call, so that the
wrapper's torch.empty most likely receives it."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import weight_image_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
KINDS = ['exact', 'rounded']
FP32_ULPS = 5
U32 = 2.0 ** -24
NAN = float('nan')


def _ops():
    from mcgen_amd import ops
    return ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _weight(shape, kind, g):
    w = torch.randn(*shape, generator=g)
    return w.bfloat16().float() if kind == 'exact' else w


def _scales(n, kind, g):
    """n scale factors: powers of two in [1/4, 4], or arbitrary values of either sign."""
    if kind == 'exact':
        return 2.0 ** torch.randint(-2, 3, (n,), generator=g).float()
    return (torch.rand(n, generator=g) * 2.5 + 0.3) * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)


def _scalar(kind, g, rounded):
    return float(2.0 ** int(torch.randint(-2, 3, (1,), generator=g))) if kind == 'exact' else rounded


def _poison(numel, dtype):
    """Leave a NaN-filled free block of this size with the caching allocator for the next torch.empty of the same size."""
    t = torch.full((numel,), NAN, dtype=dtype, device='cuda')
    torch.cuda.synchronize()
    del t


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b, what=''):
    assert a.dtype == b.dtype and a.numel() == b.numel(), what
    assert torch.equal(_bits(a).view(-1), _bits(b).view(-1)), f'{what}: {int((_bits(a).view(-1) != _bits(b).view(-1)).sum())} elements differ'


def _check(imgs, ref, kind, what=''):
    """imgs: {dtype: image tensor} with both dtypes; ref: float64 numpy of the image's shape."""
    ref = torch.from_numpy(np.ascontiguousarray(ref)).reshape(-1)
    f32 = imgs[torch.float32].cpu().reshape(-1)
    b16 = imgs[torch.bfloat16].cpu().reshape(-1)
    assert f32.numel() == ref.numel() == b16.numel(), (what, f32.numel(), ref.numel())
    if kind == 'exact':
        for name, got in (('fp32', f32), ('bf16', b16)):
            bad = (got.double() != ref).nonzero().reshape(-1)          # (NaN, an element never written, differs from everything)
            assert bad.numel() == 0, f'{what} {name}: {bad.numel()} elements differ, first at {int(bad[0])}: got {float(got[bad[0]])}, want {float(ref[bad[0]])}'
        return
    err, bound = (f32.double() - ref).abs(), FP32_ULPS * U32 * ref.abs()
    assert not torch.isnan(f32).any(), f'{what}: an element was never written'
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f'{what}: worst fp32 error = {worst * FP32_ULPS:.3f} u (bound {FP32_ULPS} u)')
    assert (err <= bound).all(), f'{what}: worst fp32 error {worst * FP32_ULPS} u; padding must be exactly zero'
    _same_bits(b16, f32.to(torch.bfloat16), f'{what}: bf16 image against the rounded fp32 image')


# ---------------------------------------------------------------------------------------------------------------------
# (Cout, Cin, ksize, transpose, row_perm): Cout in {3, 16, 24, 130}, Cin in {1, 3, 8, 33, 40, 72} (below 8, a ragged chunk,
# more than two chunks), both kernel sizes, both orientations, row_perm in {1, 2, 16} -- each value, not the product
PLAIN = [(3, 1, 1, False, 1), (16, 3, 3, False, 1), (24, 8, 3, True, 2), (130, 33, 3, False, 2), (24, 40, 1, True, 1),
         (16, 72, 3, False, 16), (130, 72, 1, True, 1), (3, 33, 3, True, 1), (16, 40, 3, True, 16), (130, 8, 3, False, 1)]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cout, cin, ks, transpose, row_perm', PLAIN)
def test_prep_weight(cout, cin, ks, transpose, row_perm, kind):
    ops, g = _ops(), _gen(cout * 1000 + cin)
    w = _weight((cout, cin, ks, ks), kind, g)
    wscale, sig = _scalar(kind, g, 0.9), _scalar(kind, g, 1.7)
    for with_sigma in (True, False):
        sigma = torch.tensor([sig]) if with_sigma else None
        imgs = {}
        for dt in DTYPES:
            out = torch.full((ops.weight_image_elems(cout, cin, ks, transpose),), NAN, dtype=dt, device='cuda')
            imgs[dt] = ops.prep_weight(w.cuda(), dt, transpose, row_perm, sigma.cuda() if with_sigma else None, wscale, out=out)
        scale = R.f32(wscale) / R.f32(sig) if with_sigma else R.f32(wscale)
        _check(imgs, R.image(w, ks, transpose=transpose, row_perm=row_perm, scale=scale), kind, f'sigma={with_sigma}')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cout, cin, ks', [(3, 1, 1), (16, 3, 3), (24, 8, 3), (130, 33, 1), (24, 40, 3), (16, 72, 1)])
def test_prep_weight_k(cout, cin, ks, kind):
    ops, g = _ops(), _gen(cout * 1000 + cin + 1)
    w = _weight((cout, cin, ks, ks), kind, g)
    wscale, sig = _scalar(kind, g, 1.3), _scalar(kind, g, 1.7)
    for with_sigma in (True, False):
        imgs = {}
        for dt in DTYPES:
            out = torch.full((ops.weight_image_k_elems(cout, cin, ks),), NAN, dtype=dt, device='cuda')
            imgs[dt] = ops.prep_weight_k(w.cuda(), dt, torch.tensor([sig]).cuda() if with_sigma else None, wscale, out=out)
        scale = R.f32(wscale) / R.f32(sig) if with_sigma else R.f32(wscale)
        _check(imgs, R.image_k(w, ks, scale), kind, f'sigma={with_sigma}')


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('cout, cin, ks', [(3, 3, 3), (24, 33, 1), (130, 40, 3), (16, 72, 3), (24, 1, 1)])
def test_prep_weight_rows(cout, cin, ks, kind):
    ops, g = _ops(), _gen(cout * 1000 + cin + 2)
    w, rs = _weight((cout, cin, ks, ks), kind, g), _scales(cout, kind, g)
    imgs = {}
    for dt in DTYPES:
        _poison(ops.weight_image_elems(cout, cin, ks), dt)
        imgs[dt] = ops.prep_weight_rows(w.cuda(), dt, rs.cuda())
        _poison(ops.weight_image_elems(cout, cin, ks), dt)
        _same_bits(imgs[dt], ops.prep_weight_ex(w.cuda(), dt, row_scale=rs.cuda()), 'prep_weight_rows against prep_weight_ex')
    _check(imgs, R.image(w, ks, row_scale=rs), kind)


# ---- the generalised builder ---------------------------------------------------------------------------------------
def _ex_cases():
    """name -> build(kind, g) -> (source view on the CPU, keyword arguments of ops.prep_weight_ex with CPU tensors)."""
    c = {}
    for t in (False, True):
        s = '-T' if t else ''
        c['full' + s] = lambda k, g, t=t: (_weight((24, 40, 3, 3), k, g), dict(transpose=t))
        # PixelCNN's vertical (2 x 3), horizontal (1 x 2) and centre (1 x 1) stacks inside a 3x3 image
        c['win23@00' + s] = lambda k, g, t=t: (_weight((24, 33, 2, 3), k, g), dict(ksize=3, transpose=t))
        c['win12@10' + s] = lambda k, g, t=t: (_weight((24, 33, 1, 2), k, g), dict(ksize=3, kh0=1, kw0=0, transpose=t))
        c['win11@11' + s] = lambda k, g, t=t: (_weight((16, 8, 1, 1), k, g), dict(ksize=3, kh0=1, kw0=1, transpose=t))
        c['linear' + s] = lambda k, g, t=t: (_weight((130, 72), k, g), dict(transpose=t))
        # strided sources, no copy
        c['rows-of-taps' + s] = lambda k, g, t=t: (_weight((24, 40, 3, 3), k, g)[:, :, :2, :], dict(ksize=3, transpose=t))
        c['channel-slice' + s] = lambda k, g, t=t: (_weight((24, 40, 3, 3), k, g)[:, 4:20], dict(transpose=t))
        c['permuted' + s] = lambda k, g, t=t: (_weight((24, 40, 3, 3), k, g).permute(1, 0, 2, 3), dict(transpose=t))
        # image extents beyond the source: forward rows = Cout, K = Cin; transposed rows = Cin, K = Cout
        c['rows_img' + s] = lambda k, g, t=t: (_weight((24, 8, 3, 3), k, g), dict(rows_img=40, transpose=t))
        c['k_img-12to16' + s] = lambda k, g, t=t: (_weight((12, 12, 3, 3), k, g), dict(k_img=16, transpose=t))
        c['k_img-40to64' + s] = lambda k, g, t=t: (_weight((40, 40, 1, 1), k, g), dict(k_img=64, transpose=t))
        c['rows_img+k_img' + s] = lambda k, g, t=t: (_weight((3, 3, 3, 3), k, g), dict(rows_img=24, k_img=40, transpose=t))
        c['scales' + s] = lambda k, g, t=t: (_weight((24, 33, 3, 3), k, g), dict(
            row_scale=_scales(24, k, g), col_scale=_scales(33, k, g), wscale=_scalar(k, g, 0.7), transpose=t))
        c['scales-win-pad' + s] = lambda k, g, t=t: (_weight((16, 3, 2, 3), k, g), dict(
            ksize=3, row_scale=_scales(16, k, g), col_scale=_scales(3, k, g), wscale=_scalar(k, g, 1.9), rows_img=40, k_img=40, transpose=t))
    return c


EX = _ex_cases()


def _ex_dev(w, kw):
    """The device view with the same strides (the whole base tensor moves, the view is re-taken) and device keyword arguments."""
    base = w._base if w._base is not None else w
    wd = base.cuda().as_strided(w.shape, w.stride(), w.storage_offset())
    return wd, {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}


def _ex_ref(w, kw):
    kw = dict(kw)
    ks = kw.pop('ksize', None)
    scale = R.f32(kw.pop('wscale', 1.0))
    return R.image(w, ks, scale=scale, **kw)


def _ex_elems(w, kw):
    t = kw.get('transpose', False)
    ks = kw.get('ksize') or (w.shape[2] if w.dim() == 4 else 1)
    rows = kw.get('rows_img') or (w.shape[1] if t else w.shape[0])
    kk = kw.get('k_img') or (w.shape[0] if t else w.shape[1])
    return _ops().weight_image_elems(rows, kk, ks, False)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', list(EX))
def test_prep_weight_ex(name, kind):
    ops = _ops()
    w, kw = EX[name](kind, _gen(len(name) + 17 * list(EX).index(name)))
    wd, kwd = _ex_dev(w, kw)
    assert wd.stride() == w.stride() and (name.split('-T')[0] not in ('rows-of-taps', 'channel-slice', 'permuted') or not wd.is_contiguous())
    imgs = {}
    for dt in DTYPES:
        _poison(_ex_elems(w, kw), dt)
        imgs[dt] = ops.prep_weight_ex(wd, dt, **kwd)
        assert imgs[dt].numel() == _ex_elems(w, kw)
        if name.startswith('full'):                         # no options: the plain builder's image
            _same_bits(imgs[dt], ops.prep_weight(wd, dt, transpose=kw['transpose']), 'prep_weight_ex against prep_weight')
    _check(imgs, _ex_ref(w, kw), kind, name)


@pytest.mark.parametrize('dt', DTYPES, ids=['fp32', 'bf16'])
def test_prep_weight_ex_many_70_jobs(dt):
    """70 jobs = 32 + 32 + 6 per launch; the largest image of each launch is its job 5, never job 0; every image is a slice
    of one NaN-filled buffer with NaN gaps between the slices."""
    from mcgen_amd._lib import CONSTANTS
    ops, g = _ops(), _gen(70)
    per = CONSTANTS['MCGEN_PREPEX_MAX']
    assert per == 32
    names = list(EX)
    big = lambda k, g: (_weight((130, 72, 3, 3), k, g), dict(row_scale=_scales(130, k, g), wscale=0.8))
    jobs_cpu = [big('rounded', g) if i % per == 5 else EX[names[(3 * i) % len(names)]]('rounded', g) for i in range(70)]
    sizes = [_ex_elems(w, kw) for w, kw in jobs_cpu]
    for base in range(0, 70, per):
        part = sizes[base:base + per]
        assert part.index(max(part)) == 5 and part.count(max(part)) == 1
    gap = 24
    buf = torch.full((sum(sizes) + gap * 71,), NAN, dtype=dt, device='cuda')
    jobs, outs, off = [], [], gap
    for (w, kw), n in zip(jobs_cpu, sizes):
        wd, kwd = _ex_dev(w, kw)
        outs.append(buf[off:off + n])
        jobs.append((wd, dict(kwd, out=outs[-1])))
        off += n + gap
    got = ops.prep_weight_ex_many(jobs, dt)
    torch.cuda.synchronize()
    live = torch.zeros(buf.numel(), dtype=torch.bool)
    off = gap
    for i, ((wd, kwd), n) in enumerate(zip(jobs, sizes)):
        assert got[i].data_ptr() == outs[i].data_ptr()
        kwd = {k: v for k, v in kwd.items() if k != 'out'}
        _same_bits(got[i], ops.prep_weight_ex(wd, dt, **kwd), f'job {i} against the single call')
        live[off:off + n] = True
        off += n + gap
    host = buf.cpu()
    assert torch.isnan(host[~live]).all(), 'a gap between the images was written'
    assert not torch.isnan(host[live]).any(), 'an image element was never written'


# ---- the batched builder -------------------------------------------------------------------------------------------------
def _prep_jobs(kind, g):
    """The mixed table: (weight, transpose, row_perm, sigma_idx, wscale, kmajor, kmap, kcount, rmap), CPU tensors."""
    ws = lambda r: _scalar(kind, g, r)
    w2440 = _weight((24, 40, 3, 3), kind, g)

    def kmap(kcount, live):
        """`live` distinct source channels in random order, then -1 and Cin = 40 (zero columns) up to kcount, with one more zero
        column in the middle; the eight entries past kcount name a real channel and must not be read."""
        m = torch.randperm(40, generator=g)[:live].tolist()
        m = m[:live // 2] + [40] + m[live // 2:]
        m = (m + [-1] + [40] * kcount)[:kcount] + [7] * 8
        return torch.tensor(m, dtype=torch.int16)

    return [
        (w2440, False, 1, -1, 1.0, False, None, 0, None),
        (w2440, True, 2, 0, ws(2.1), False, None, 0, None),
        (_weight((16, 72, 1, 1), kind, g), False, 16, 2, ws(0.6), False, None, 0, None),
        (_weight((130, 33, 3, 3), kind, g), False, 1, 1, 1.0, False, None, 0, None),
        (_weight((24, 33, 3, 3), kind, g), False, 1, 1, ws(1.4), True, None, 0, None),          # K-major
        (w2440, False, 1, 2, 1.0, False, kmap(8, 5), 8, None),
        (w2440, False, 1, -1, ws(0.3), False, kmap(24, 21), 24, None),
        (w2440, False, 1, 0, 1.0, False, kmap(40, 33), 40, None),
        (_weight((24, 8, 3, 3), kind, g), False, 1, 1, 1.0, False, None, 0, torch.randperm(24, generator=g).to(torch.int16)),
        (_weight((130, 72), kind, g), True, 1, 0, ws(1.1), False, None, 0, None),
        (w2440, False, 1, 1, 1.0, False, kmap(24, 17), 24, torch.randperm(24, generator=g).to(torch.int16)),
        (_weight((3, 1, 3, 3), kind, g), True, 1, -1, 1.0, False, None, 0, None),
    ]


def _prep_elems(job):
    ops = _ops()
    w, transpose, _, _, _, kmajor, kmap, kcount, _ = job
    cout, cin, ks = w.shape[0], w.shape[1], (w.shape[2] if w.dim() == 4 else 1)
    if kmajor:
        return ops.weight_image_k_elems(cout, cin, ks)
    return ops.weight_image_elems(cout, kcount if kmap is not None else cin, ks, transpose)


def _prep_batch(jobs, dt):
    """-> (PrepBatch, [image tensors], the device tensors to keep alive)."""
    ops = _ops()
    dev = lambda t: None if t is None else t.cuda()
    table, imgs, keep = [], [], []
    for job in jobs:
        w, transpose, row_perm, sidx, wscale, kmajor, kmap, kcount, rmap = job
        img = torch.full((_prep_elems(job),), NAN, dtype=dt, device='cuda')
        wd, km, rm = dev(w), dev(kmap), dev(rmap)
        keep += [wd, km, rm]
        imgs.append(img)
        table.append(ops.PrepJob(wd, img, transpose, row_perm, sidx, wscale, kmajor, km, kcount, rm))
    return ops.PrepBatch(table, dt), imgs, keep


def _prep_ref(job, sigma):
    w, transpose, row_perm, sidx, wscale, kmajor, kmap, kcount, rmap = job
    ks = w.shape[2] if w.dim() == 4 else 1
    scale = R.f32(wscale) / float(sigma[sidx]) if sidx >= 0 else R.f32(wscale)
    if kmajor:
        return R.image_k(w, ks, scale)
    return R.image(w, ks, transpose=transpose, row_perm=row_perm, scale=scale, kmap=kmap, kcount=kcount, rmap=rmap)


def _sigma(kind):
    return torch.tensor([0.5, 4.0, 2.0] if kind == 'exact' else [1.7, 0.6, 2.3])


@pytest.mark.parametrize('kind', KINDS)
def test_prep_batch_mixed_table(kind):
    ops = _ops()
    jobs, sigma = _prep_jobs(kind, _gen(5)), _sigma(kind)
    assert {j[7] for j in jobs} >= {8, 24, 40} and any(j[5] for j in jobs) and {j[3] for j in jobs} == {-1, 0, 1, 2}
    sd = sigma.cuda()
    imgs = {}
    for dt in DTYPES:
        pb, imgs[dt], keep = _prep_batch(jobs, dt)
        pb.run(sd)
        torch.cuda.synchronize()
        for i, (job, img) in enumerate(zip(jobs, imgs[dt])):
            w, transpose, row_perm, sidx, wscale, kmajor, kmap, kcount, rmap = job
            if kmap is not None or rmap is not None:
                continue                                     # (no single-call builder takes these maps)
            s1 = sd[sidx:sidx + 1] if sidx >= 0 else None
            single = ops.prep_weight_k(w.cuda(), dt, s1, wscale) if kmajor else ops.prep_weight(w.cuda(), dt, transpose, row_perm, s1, wscale)
            _same_bits(img, single, f'job {i} against the single-call builder')
    for i, job in enumerate(jobs):
        _check({dt: imgs[dt][i] for dt in DTYPES}, _prep_ref(job, sigma.double()), kind, f'job {i}')


@pytest.mark.parametrize('kind', KINDS)
def test_prep_batch_block_stride_loop_goes_round_twice(kind):
    """Cout 528, Cin 128, 1x1: 66 row groups x 4 chunks = 264 groups of 8 rows x 32 columns for the 256 blocks an image gets."""
    ops, g = _ops(), _gen(528)
    job = (_weight((528, 128, 1, 1), kind, g), False, 1, 0, _scalar(kind, g, 0.9), False, None, 0, None)
    assert (R.round_up(528, 16) // 8) * R.chunks(128) == 264 > 256
    sigma = _sigma(kind)
    imgs = {}
    for dt in DTYPES:
        pb, (img,), keep = _prep_batch([job], dt)
        pb.run(sigma.cuda())
        torch.cuda.synchronize()
        imgs[dt] = img
        _same_bits(img, ops.prep_weight(job[0].cuda(), dt, False, 1, sigma[:1].cuda(), job[4]), 'against prep_weight')
    _check(imgs, _prep_ref(job, sigma.double()), kind)


@pytest.mark.parametrize('dt', DTYPES, ids=['fp32', 'bf16'])
def test_prep_and_codes_equals_the_two_launches(dt):
    ops, g = _ops(), _gen(9)
    jobs, sigma = _prep_jobs('rounded', g), _sigma('rounded').cuda()
    pb_a, imgs_a, keep_a = _prep_batch(jobs, dt)
    pb_b, imgs_b, keep_b = _prep_batch(jobs, dt)
    modes = 10
    books = [torch.randn(modes, c, generator=g) for c in (8, 36, 132, 4)]
    codes = ops.CodeBatch([SimpleNamespace(codebook=b.cuda()) for b in books], scale_idx=[0, -1, 1, 1])
    label = torch.tensor([3, 0, 9, 9, 4], dtype=torch.int64)
    scale = torch.tensor([1.7, 0.45])
    reps, n_half = 2, 5
    fused = ops.prep_and_codes(pb_a, sigma, codes, label.cuda(), reps, scale.cuda(), n_half)
    fused = [c.clone() for c in fused]
    pb_b.run(sigma)
    apart = codes.run_labels(label.cuda(), reps, scale.cuda(), n_half)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(imgs_a, imgs_b)):
        assert not torch.isnan(a.float()).any()
        _same_bits(a, b, f'image {i}')
    sidx = [0, -1, 1, 1]
    for i, (a, b, book) in enumerate(zip(fused, apart, books)):
        assert a.shape == (reps * 5, book.shape[1])
        _same_bits(a, b, f'codes {i}')
        want = book[label.repeat(reps)]
        if sidx[i] >= 0:
            want[n_half:] = want[n_half:] * scale[sidx[i]]          # one fp32 multiplication, as the kernel's
        assert torch.equal(a.cpu(), want), f'codes {i} against codebook[label]'


# ---- layout converters --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c, cp', [(1, 8), (3, 8), (12, 16), (8, 8)])
def test_layout_converters(c, cp):
    ops, g = _ops(), _gen(c)
    n, h, w = 2, 3, 5
    x = torch.randn(n, c, h, w, generator=g)
    # ties of the bf16 rounding (8 significant bits): exactly halfway, to the even and to the odd neighbour, both signs,
    # and one that carries into the exponent
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 2 - 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20,
                         1 + 2.0 ** -8 - 2.0 ** -20])
    x.view(-1)[:ties.numel()] = ties
    x.view(-1)[-ties.numel():] = ties.flip(0) * 0.5
    for dt in DTYPES:
        out = torch.full((n, h, w, cp), NAN, dtype=dt, device='cuda')
        y = ops.to_nhwc(x.cuda(), dt, cp, out=out)
        assert y.data_ptr() == out.data_ptr()
        want = torch.zeros(n, h, w, cp, dtype=dt)
        want[..., :c] = x.permute(0, 2, 3, 1).to(dt)              # (torch's conversion is round-to-nearest-even)
        _same_bits(y.cpu(), want, f'to_nhwc {dt}')
        assert (y.cpu()[..., c:] == 0).all()
        _poison(x.numel(), torch.float32)
        back = ops.to_nchw(y, c)
        assert torch.equal(back.cpu(), x.to(dt).float()), f'to_nchw {dt}'
    xb = x.bfloat16().float()                                     # bf16-representable data survives the round trip in both dtypes
    for dt in DTYPES:
        assert torch.equal(ops.to_nchw(ops.to_nhwc(xb.cuda(), dt, cp), c).cpu(), xb)
