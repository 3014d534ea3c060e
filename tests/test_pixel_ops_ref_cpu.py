"""The float64 references of tests/pixel_ops_ref.py against torch's own float64 operators and autograd (no GPU), and the
host-side refusals of the entry points of csrc/pixelcnn_ops.hip and csrc/vq_ops.hip, which return before any launch."""
import os

import pytest
import torch
import torch.nn.functional as F

import pixel_ops_ref as R

F64 = torch.float64
TOL = 1e-12


def _close(a, b, tol=TOL):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max())), float((a - b).abs().max())


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _w_taps(w):
    """Conv weight [Cout, Cin, kh, kw] -> the matrix [kh * kw * Cin, Cout] that multiplies an im2col row."""
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0])


# ---- im2col / col2im ------------------------------------------------------------------------------------------------
GEOMS = [(4, 7, 3, 3, 1), (1, 4, 0, 3, 1), (2, 3, 1, 1, 1), (1, 2, 0, 1, 1), (3, 3, 1, 1, 1), (4, 4, 1, 1, 2)]


@pytest.mark.parametrize('kh,kw,oh,ow,stride', GEOMS)
def test_im2col_is_conv2d(kh, kw, oh, ow, stride):
    """im2col(x) @ W equals F.conv2d on the input padded by (oh, ow) before and whatever the taps need after; with the
    prologue the padding is applied to the activated tensor."""
    gen = torch.Generator().manual_seed(kh * 10 + kw)
    n, h, w, c, co = 3, 6, 10, 5, 4
    x = torch.randn(n, h, w, c, generator=gen, dtype=F64)
    wt = torch.randn(co, c, kh, kw, generator=gen, dtype=F64)
    sc, sh = torch.randn(c, generator=gen, dtype=F64), torch.randn(c, generator=gen, dtype=F64)
    code = torch.randn(n, c, generator=gen, dtype=F64)
    for args in ({}, {'scale': sc, 'shift': sh}, {'relu': True}, {'code': code},
                 {'scale': sc, 'shift': sh, 'relu': True, 'code': code}):
        col = R.im2col(x, kh, kw, oh, ow, stride, **args)
        ho, wo = h // stride, w // stride
        assert col.shape == (n, ho, wo, kh * kw * c)
        act = R.activate(x, **args)
        pb, pr = (ho - 1) * stride + kh - oh - h, (wo - 1) * stride + kw - ow - w
        xp = F.pad(_nchw(act), (ow, max(pr, 0), oh, max(pb, 0)))
        ref = _nhwc(F.conv2d(xp, wt, stride=stride))[:, :ho, :wo]
        _close(col @ _w_taps(wt), ref)
    act = R.activate(x, sc, sh, True, code)
    _close(act, torch.relu(x * sc + sh) * code[:, None, None, :])
    assert float((act - torch.relu((x * sc + sh) * code[:, None, None, :])).abs().max()) > 0.1     # the order matters


@pytest.mark.parametrize('kh,kw,oh,ow,stride', GEOMS)
def test_col2im_is_the_adjoint(kh, kw, oh, ow, stride):
    """<im2col(x), y> = <x, col2im(y)> for every geometry, elementwise through autograd; bias only on channels < C;
    base is added as it stands."""
    gen = torch.Generator().manual_seed(kh * 10 + kw + 1)
    n, h, w, cp = 2, 6, 10, 8
    x = torch.randn(n, h, w, cp, generator=gen, dtype=F64, requires_grad=True)
    y = torch.randn(n, h // stride, w // stride, kh * kw * cp, generator=gen, dtype=F64)
    (R.im2col(x, kh, kw, oh, ow, stride) * y).sum().backward()
    _close(R.col2im(y, cp, kh, kw, oh, ow, stride), x.grad)
    bias = torch.randn(3, generator=gen, dtype=F64)
    withb = R.col2im(y, cp, kh, kw, oh, ow, stride, bias=bias)
    _close(withb[..., :3], x.grad[..., :3] + bias)
    _close(withb[..., 3:], x.grad[..., 3:])
    base = torch.randn(n, h, w, cp, generator=gen, dtype=F64)
    _close(R.col2im(y, cp, kh, kw, oh, ow, stride, bias=bias, base=base), x.grad + base)


def test_col2im_is_conv_transpose2d():
    """nn.ConvTranspose2d(Cin, Cout, 4, 2, 1): col2im of x @ W with 4x4 taps, stride 2, offsets 1 (mcvae.py:89,95)."""
    gen = torch.Generator().manual_seed(5)
    n, hi, wi, cin, cout = 2, 3, 5, 6, 8
    x = torch.randn(n, hi, wi, cin, generator=gen, dtype=F64)
    wt = torch.randn(cin, cout, 4, 4, generator=gen, dtype=F64)
    bias = torch.randn(cout, generator=gen, dtype=F64)
    dcol = x @ wt.permute(0, 2, 3, 1).reshape(cin, 16 * cout)
    got = R.col2im(dcol, cout, 4, 4, 1, 1, 2, bias=bias)
    _close(got, _nhwc(F.conv_transpose2d(_nchw(x), wt, bias, stride=2, padding=1)))


# ---- gated activation and the tails, through F.batch_norm and autograd --------------------------------------------------
def _bn_case(shape, gen):
    x = torch.randn(*shape, generator=gen, dtype=F64) * 1.5 + 0.3
    c = shape[-1]
    gamma, beta = torch.randn(c, generator=gen, dtype=F64), torch.randn(c, generator=gen, dtype=F64)
    eps = 1e-5
    flat = x.reshape(-1, c)
    mean, var = flat.mean(0), flat.var(0, unbiased=False)
    rstd = 1 / torch.sqrt(var + eps)
    scale = gamma * rstd
    return x, gamma, beta, eps, mean, rstd, scale, beta - mean * scale


def _bn(x, gamma, beta, eps):
    return _nhwc(F.batch_norm(_nchw(x), None, None, gamma, beta, training=True, eps=eps))


def test_gated_forward_and_backward_match_autograd():
    gen = torch.Generator().manual_seed(11)
    n, h, w, c = 3, 4, 5, 6
    a, gamma, beta, eps, mean, rstd, scale, shift = _bn_case((n, h, w, c), gen)
    b = torch.randn(n, h, w, c, generator=gen, dtype=F64) * 2
    code = torch.randn(n, c, generator=gen, dtype=F64)
    g = torch.randn(n, h, w, c, generator=gen, dtype=F64)
    s = torch.cat([a, b], -1).requires_grad_(True)
    gamma.requires_grad_(True), beta.requires_grad_(True)
    out = code[:, None, None, :] * torch.relu(_bn(s[..., :c], gamma, beta, eps)) * torch.sigmoid(s[..., c:])
    _close(R.gated_fwd(s.detach(), scale.detach(), shift.detach(), code), out.detach())
    (out * g).sum().backward()
    ds, dgamma, dbeta = R.gated_bwd(s.detach(), scale.detach(), shift.detach(), mean, rstd, code, g)
    _close(ds, s.grad, 1e-11)
    _close(dgamma, gamma.grad, 1e-11)
    _close(dbeta, beta.grad, 1e-11)
    seen = []
    R.gated_bwd(s.detach(), scale.detach(), shift.detach(), mean, rstd, code, g, round_dz=lambda t: seen.append(t) or t)
    assert len(seen) == 1 and seen[0].shape == (n, h, w, c)


@pytest.mark.parametrize('use_code', [False, True])
@pytest.mark.parametrize('use_res', [False, True])
@pytest.mark.parametrize('pre_relu', [False, True])
@pytest.mark.parametrize('post_relu', [False, True])
def test_tail_forward_and_backward_match_autograd(use_code, use_res, pre_relu, post_relu):
    gen = torch.Generator().manual_seed(12 + use_code + 2 * use_res + 4 * pre_relu + 8 * post_relu)
    n, h, w, c = 3, 4, 5, 6
    x, gamma, beta, eps, mean, rstd, scale, shift = _bn_case((n, h, w, c), gen)
    code = torch.randn(n, c, generator=gen, dtype=F64) if use_code else None
    res = torch.randn(n, h, w, c, generator=gen, dtype=F64) if use_res else None
    g = torch.randn(n, h, w, c, generator=gen, dtype=F64)
    x.requires_grad_(True), gamma.requires_grad_(True), beta.requires_grad_(True)
    if use_res:
        res.requires_grad_(True)
    z = _bn(x, gamma, beta, eps)
    z = torch.relu(z) if pre_relu else z
    z = z * code[:, None, None, :] if use_code else z
    z = z + res if use_res else z
    y = torch.relu(z) if post_relu else z
    _close(R.affine_code_res(x.detach(), scale.detach(), shift.detach(), code, None if res is None else res.detach(),
                             pre_relu, post_relu), y.detach())
    (y * g).sum().backward()
    dx, dgamma, dbeta, gg = R.code_bn_bwd(g, code, x.detach(), scale.detach(), mean, rstd, shift=shift.detach(),
                                          pre_relu=pre_relu, y_post=y.detach() if post_relu else None)
    _close(dx, x.grad, 1e-11)
    _close(dgamma, gamma.grad, 1e-11)
    _close(dbeta, beta.grad, 1e-11)
    if use_res:
        _close(gg, res.grad)
    if post_relu:
        assert torch.equal(gg, g * (y.detach() > 0))
    else:
        assert torch.equal(gg, g)


def test_affine_relu_maxpool2_is_max_pool2d():
    gen = torch.Generator().manual_seed(13)
    x = torch.randn(2, 6, 10, 8, generator=gen, dtype=F64)
    sc, sh = torch.randn(8, generator=gen, dtype=F64), torch.randn(8, generator=gen, dtype=F64) - 0.5
    ref = _nhwc(F.max_pool2d(torch.relu(_nchw(x * sc + sh)), 2))
    got = R.affine_relu_maxpool2(x, sc, sh)
    assert torch.equal(got, ref) and (got == 0).any() and (sc < 0).any()


# ---- losses -----------------------------------------------------------------------------------------------------------
def test_bce_matches_binary_cross_entropy_where_both_agree():
    """|a| <= 30.  F.binary_cross_entropy(sigmoid(a)) rounds sigmoid(a) to 53 bits first; next to 1 that is an absolute
    error of 2^-53, which log(1 - s) divides by 1 - s >= exp(-|a|): the two forms agree to 2^-52 exp(|a|) (1e-3 at 30, 5e-9 at
    18) plus rounding, and that is the bound here.  torch's backward divides by max(s (1 - s), 1e-12), which is exact only
    for |a| < 27, so the gradient is compared for |a| <= 25.  Above 37 the sigmoid form has saturated to the clamp: at
    a = 40, t = 0 it gives 100, the reference 40."""
    gen = torch.Generator().manual_seed(14)
    a = (torch.rand(4000, generator=gen, dtype=F64) * 60 - 30).requires_grad_(True)
    t = torch.rand(4000, generator=gen, dtype=F64)
    t[:100], t[100:200] = 0.0, 1.0
    ref = F.binary_cross_entropy(torch.sigmoid(a), t, reduction='none')
    ref.sum().backward()
    r, loss, d = R.bce_logits(a.detach(), t, 0.5)
    _close(r, torch.sigmoid(a.detach()))
    amp = 2.0 ** -52 * torch.exp(a.detach().abs())
    assert bool(((loss - ref.detach()).abs() <= amp + 1e-12 * (1 + loss)).all())
    near = a.detach().abs() <= 18
    assert int(near.sum()) > 1000 and float((loss - ref.detach()).abs()[near].max()) < 1e-8
    low = a.detach().abs() <= 25
    assert bool(((d - 0.5 * a.grad).abs()[low] <= (amp + 1e-12)[low]).all())
    big = torch.tensor([40.0, -40.0, 200.0, -200.0, 200.0, -200.0], dtype=F64)
    tt = torch.tensor([0.0, 1.0, 0.0, 1.0, 1.0, 0.0], dtype=F64)
    _close(R.bce_logits(big, tt)[1], torch.tensor([40.0, 40.0, 100.0, 100.0, 0.0, 0.0], dtype=F64), 1e-15)
    assert float(F.binary_cross_entropy(torch.sigmoid(big[:1]), tt[:1])) == 100.0
    _close(R.softplus(torch.tensor([0.0, 3.0], dtype=F64)), F.softplus(torch.tensor([0.0, 3.0], dtype=F64)))


def test_cross_entropy_matches_torch():
    gen = torch.Generator().manual_seed(15)
    p, c = 37, 65
    x = (torch.randn(p, c, generator=gen, dtype=F64) * 20).requires_grad_(True)
    with torch.no_grad():
        x[3] = 1.25
        x[4, 10:20] = float('-inf')
    tgt = torch.randint(0, c, (p,), generator=gen)
    tgt[4] = 64
    ref = F.cross_entropy(x, tgt, reduction='none')
    ref.mean().backward()
    rows, dl = R.cross_entropy(x.detach(), tgt, 1.0 / p)
    _close(rows, ref.detach())
    _close(dl, x.grad)
    assert abs(float(rows[3]) - float(torch.log(torch.tensor(65.0, dtype=F64)))) < 1e-12


def test_argmin_matches_torch_argmin():
    gen = torch.Generator().manual_seed(16)
    inf, nan = float('inf'), float('nan')
    x = torch.randn(64, 100, generator=gen, dtype=F64)
    x[0] = inf
    x[1] = nan
    x[2, 40], x[2, 70] = nan, nan
    x[3, 5], x[3, 69] = -inf, -inf
    x[4] = inf
    x[4, 99] = 1e300
    x[5, 17], x[5, 81] = -9.0, -9.0
    x[6] = 0.0
    x[6, 30], x[6, 31] = -0.0, 0.0
    x[7] = 1.0
    x[7, 50], x[7, 20] = 0.0, -0.0
    x[8, 3], x[8, 60] = -inf, nan
    x[9] = -inf
    got = R.argmin(x)
    assert torch.equal(got, torch.argmin(x, -1))
    assert got[:10].tolist() == [0, 0, 40, 5, 99, 17, 0, 20, 60, 0]
    b = torch.randn(50, 512, generator=gen).bfloat16()                       # bf16: many exact ties
    assert torch.equal(R.argmin(b), torch.argmin(b.float(), -1))
    assert torch.equal(R.argmin(x[:, :1]), torch.zeros(64, dtype=torch.int64))


def test_mse_tanh_matches_torch():
    gen = torch.Generator().manual_seed(17)
    x = (torch.randn(5, 7, 3, generator=gen, dtype=F64) * 3).requires_grad_(True)
    t = torch.rand(5, 7, 3, generator=gen, dtype=F64) * 2 - 1
    loss = F.mse_loss(torch.tanh(x), t)
    loss.backward()
    r, sse, dx = R.mse_tanh(x.detach(), t, 2.0 / x.numel())
    _close(r, torch.tanh(x.detach()))
    _close(sse / x.numel(), loss.detach())
    _close(dx, x.grad)


def test_vq_step_matches_the_module_statements():
    """modules.py:18-43 restated with index_add / bincount instead of the one-hot matrix products."""
    gen = torch.Generator().manual_seed(18)
    p, d, k = 300, 24, 64
    emb = torch.randn(d, k, generator=gen, dtype=F64)
    codes = torch.randint(0, k, (p,), generator=gen)
    codes[codes == 7] = 8
    feat = emb[:, codes].t() + 0.1 * torch.randn(p, d, generator=gen, dtype=F64)
    cs0 = torch.rand(k, generator=gen, dtype=F64) * 3
    mean0 = torch.randn(d, k, generator=gen, dtype=F64)
    r = R.vq_step(feat, codes, emb, cs0, mean0, 0.99, 0.01, 1e-5, 0.25)
    cnt = torch.bincount(codes, minlength=k).double()
    sums = torch.zeros(k, d, dtype=F64).index_add_(0, codes, feat).t()
    cs = 0.99 * cs0 + 0.01 * cnt
    em = 0.99 * mean0 + 0.01 * sums
    n = cs.sum()
    _close(r['counts'], cnt), _close(r['cs'], cs), _close(r['em'], em)
    _close(r['e'], em / ((cs + 1e-5) / (n + k * 1e-5) * n))
    assert r['counts'][7] == 0
    f = feat.clone().requires_grad_(True)
    q = F.embedding(codes, emb.t())
    diff = F.mse_loss(q, f)
    (0.25 * diff).backward()
    _close(r['q'], q), _close(r['diff'], diff.detach()), _close(r['g'], f.grad)


# ---- host refusals: every entry point checks its arguments before it launches anything ----------------------------------
@pytest.fixture(scope='module')
def lib():
    from mcgen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


_BUF = torch.zeros(64)
P = _BUF.data_ptr()          # a non-null address: the refused calls never pass it on


def _refused(lib, rc, text):
    assert rc != 0
    assert text.encode() in lib.mcgen_last_error(), lib.mcgen_last_error()


@pytest.mark.parametrize('c', [24, 4096])
def test_stats_kernels_refuse_channel_counts_that_do_not_divide_the_block(lib, c):
    """C / 8 must divide 256: 24 gives 3 groups, 4096 gives 512 groups for 256 threads."""
    _refused(lib, lib.mcgen_gated_bwd_stats(P, P, P, P, P, P, P, P, P, 4, 0, 2, 16, c, None), 'gated_bwd_stats: C/8 must divide 256')
    _refused(lib, lib.mcgen_code_bn_stats(P, P, P, P, P, P, P, 4, 0, 2, 16, c, P, P, 0, None, None, None),
             'code_bn_stats: C/8 must divide 256')


def test_code_bn_stats_refuses_pre_relu_without_the_affine(lib):
    _refused(lib, lib.mcgen_code_bn_stats(P, P, P, P, P, P, P, 4, 0, 2, 16, 16, None, None, 1, None, None, None), 'needs the BatchNorm affine')
    _refused(lib, lib.mcgen_code_bn_stats(P, P, P, P, P, P, P, 4, 0, 2, 16, 16, P, None, 1, None, None, None), 'needs the BatchNorm affine')


def test_im2col_col2im_refusals(lib):
    _refused(lib, lib.mcgen_im2col(P, P, 0, 2, 6, 10, 12, 3, 3, 1, 1, 1, None, None, 0, None, None), 'im2col: bad arguments')
    _refused(lib, lib.mcgen_col2im(P, P, 0, 2, 6, 10, 12, 3, 3, 1, 1, 1, None, 0, 0, None), 'col2im: bad arguments')
    _refused(lib, lib.mcgen_im2col(P, P, 0, 2, 7, 10, 8, 4, 4, 1, 1, 2, None, None, 0, None, None), 'im2col: bad arguments')
    _refused(lib, lib.mcgen_im2col(P, P, 0, 2, 6, 9, 8, 4, 4, 1, 1, 2, None, None, 0, None, None), 'im2col: bad arguments')
    _refused(lib, lib.mcgen_col2im(P, P, 0, 2, 7, 10, 8, 4, 4, 1, 1, 2, None, 0, 0, None), 'col2im: bad arguments')
    _refused(lib, lib.mcgen_im2col(P, P, 0, 2, 6, 10, 8, 3, 3, 1, 1, 1, P, None, 0, None, None), 'scale and shift come together')
    _refused(lib, lib.mcgen_im2col(P, P, 0, 2, 6, 10, 8, 3, 3, 1, 1, 1, None, P, 0, None, None), 'scale and shift come together')
    _refused(lib, lib.mcgen_im2col(P, P, 7, 2, 6, 10, 8, 3, 3, 1, 1, 1, None, None, 0, None, None), 'bad dtype')


@pytest.mark.parametrize('n', [0, 5])
def test_gated_fwd_batch_refuses_job_counts_outside_the_cap(lib, n):
    from mcgen_amd import _lib as L
    jobs = (L.Gated * 8)()
    for j in jobs:
        j.s = j.scale = j.shift = j.code = j.out = P
        j.N, j.HW, j.C = 1, 4, 8
    _refused(lib, lib.mcgen_gated_fwd_batch(jobs, n, 0, None), 'gated_fwd_batch: 1 .. 4 gates')


def test_vq_stats_refusals(lib):
    args = lambda d, fp, k: (P, P, P, P, P, P, P, P, 1.0, 0, 100, d, fp, k, 1, None)          # noqa: E731
    _refused(lib, lib.mcgen_vq_stats(*args(72, 72, 64)), 'vq_stats: D must be a multiple of 8 up to 64')
    _refused(lib, lib.mcgen_vq_stats(*args(12, 16, 64)), 'vq_stats: D must be a multiple of 8 up to 64')
    _refused(lib, lib.mcgen_vq_stats(*args(16, 16, 96)), 'vq_stats: K must be a multiple of 64')
    _refused(lib, lib.mcgen_vq_stats(P, P, P, P, P, None, None, P, 1.0, 0, 100, 16, 16, 64, 1, None), 'training needs the statistics slabs')


def test_loss_kernels_refuse_more_than_4096_blocks(lib):
    _refused(lib, lib.mcgen_bce_logits(P, P, P, P, P, 4097, 1.0, 0, 100, 3, 8, None), 'bce_logits: bad arguments')
    _refused(lib, lib.mcgen_mse_tanh(P, P, P, P, P, 4097, 1.0, 0, 100, 3, 8, None), 'mse_tanh: bad arguments')
    _refused(lib, lib.mcgen_mse_tanh(P, P, P, P, P, 16, 1.0, 0, 100, 3, 12, None), 'mse_tanh: bad arguments')
