"""GPU tests of the kernels of csrc/glow_variants.hip against float64 on the host: the float64 factorisation of the plain
InvConv2d weight (log|det W| and W^-1, single and batched), its weight gradient dW + ld_coef W^-T, and additive coupling.
Bounds are derived from the number formats (u64 = 2^-53, u32 = 2^-24, bf16 2^-8) and the matrix's condition number, in the
style of test_mcglow_kernels_gpu.py::test_invconv_weight_and_inverse; none is tuned to what the kernels return."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U64, U32, UBF = 2.0 ** -53, 2.0 ** -24, 2.0 ** -8
SIZES = [1, 2, 3, 4, 12, 24, 48, 53, 64]


def _matrices(c, seed):
    """fp32 [C, C] test matrices: a random orthogonal matrix times a diagonal with entries in [0.5, 2]; the same with a
    negative determinant; one whose leading entry is exactly 0 (the first pivot has to come from another row)."""
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(c, c, generator=g, dtype=torch.float64))
    w = (q * (0.5 + 1.5 * torch.rand(c, generator=g, dtype=torch.float64))).float().contiguous()     # (qr returns column-major)
    neg = w.clone()
    if torch.linalg.slogdet(neg.double())[0] > 0:
        neg[0] = -neg[0]
    out = [('orthogonal x diagonal', w), ('negative determinant', neg)]
    if c > 1:
        lead = w.clone(); lead[0, 0] = 0.0
        out.append(('zero leading entry', lead))
    return out


def _reference(w):
    wd = w.double()
    sign, lad = torch.linalg.slogdet(wd)
    inv = torch.linalg.inv(wd)
    cond = float(torch.linalg.norm(wd) * torch.linalg.norm(inv))
    return float(sign), float(lad), inv, cond


def _inv_bound(c, cond, inv):
    """Gauss-Jordan with partial pivoting in float64 is backward stable up to a growth factor that is O(1) on these matrices:
    the forward error of the inverse is at most ~ C u64 cond (8 C as the constant); + one rounding to fp32."""
    return (8 * c * U64 * cond + U32) * float(torch.linalg.norm(inv))


def _check_factorisation(name, w, lad, winv):
    c = w.shape[0]
    sign, ref, inv, cond = _reference(w)
    err_inv = float(torch.linalg.norm(winv.double().cpu() - inv))
    err_lad = abs(float(lad) - ref)
    tol_lad = U32 * abs(ref) + 8 * c * c * U64 * cond        # C pivots, each with relative error <= ~ 8 C u64 cond; one rounding
    print(f'C={c} {name}: cond_F {cond:.3g} |dX|_F {err_inv:.3g} (bound {_inv_bound(c, cond, inv):.3g}) '
          f'|dlogdet| {err_lad:.3g} (bound {tol_lad:.3g})')
    assert err_inv <= _inv_bound(c, cond, inv), (name, c)
    assert err_lad <= tol_lad, (name, c)
    return sign


@pytest.mark.parametrize('c', SIZES)
def test_invconv_plain_single(c):
    from mcgen_amd import ops
    signs = []
    for name, w in _matrices(c, 100 + c):
        wd = w.cuda()
        lad, winv = ops.invconv_plain(wd)
        assert lad.shape == (1,) and winv.shape == (c, c) and lad.dtype == winv.dtype == torch.float32
        signs.append(_check_factorisation(name, w, lad, winv))
        lad4, winv4 = ops.invconv_plain(wd.view(c, c, 1, 1))                  # the parameter's own shape, read densely
        assert torch.equal(lad4, lad) and torch.equal(winv4, winv)
        assert torch.equal(wd.cpu(), w)                                      # the weight is only read
    assert -1.0 in signs                                                     # the sign plays no part in log|det|


def test_invconv_plain_batch_mixed_sizes():
    """One call with every size and matrix kind mixed: more jobs than MCGEN_GLOW_BATCH_MAX, so more than one launch, and the
    LDS of a launch sized by its largest job.  Bit-identical to the single form."""
    from mcgen_amd import _lib, ops
    cases = [(c, name, w) for c in SIZES for name, w in _matrices(c, 100 + c)]
    cases = cases[1::2] + cases[0::2]                                        # sizes interleaved across the launches
    assert len(cases) > _lib.CONSTANTS['MCGEN_GLOW_BATCH_MAX']
    ws = [w.cuda() for _, _, w in cases]
    out = ops.invconv_plain_batch(ws)
    assert len(out) == len(cases)
    for (c, name, w), wd, (lad, winv) in zip(cases, ws, out):
        _check_factorisation(name, w, lad, winv)
        lad1, winv1 = ops.invconv_plain(wd)
        assert torch.equal(lad1, lad) and torch.equal(winv1, winv), (c, name)


@pytest.mark.parametrize('c', [1, 3, 24, 64])
def test_invconv_plain_singular(c):
    """An all-zero row: the elimination keeps it exactly zero, a pivot is exactly 0, logabsdet is -inf as torch.slogdet's;
    the call returns normally and the inverse is not finite.  In a batch the other jobs are untouched."""
    from mcgen_amd import ops
    w = _matrices(c, 7)[0][1]
    w[c // 2] = 0.0
    assert float(torch.linalg.slogdet(w.double())[1]) == float('-inf')
    lad, winv = ops.invconv_plain(w.cuda())
    torch.cuda.synchronize()
    assert float(lad) == float('-inf')
    assert not bool(torch.isfinite(winv).any())
    good = _matrices(c, 8)[0][1]
    out = ops.invconv_plain_batch([good.cuda(), w.cuda(), good.cuda()])
    assert float(out[1][0]) == float('-inf')
    for k in (0, 2):
        _check_factorisation('next to a singular job', good, *out[k])


def _bwd_case(c, ldw, accumulate, seed):
    g = torch.Generator().manual_seed(seed)
    w = _matrices(c, 100 + c)[-1][1]
    dW = torch.randn(c, ldw, generator=g)                                   # columns >= C: the padded part of the 1x1 gradient
    g0 = torch.randn(c, c, 1, 1, generator=g)
    return w, dW, g0


def _bwd_check(w, dW, g0, accumulate, ld_coef, got):
    """float64 autograd of <W, dW> + ld_coef log|det W|; the kernel adds ld_coef * X^T (X the kernel's fp32 inverse) to dW
    in one fused multiply-add (one rounding) and, accumulating, to the old value (one more): elementwise
    |err| <= |ld_coef| |X - W^-1|_F + u32 (2 |ref| + |g0|) with the inverse's bound above."""
    c = w.shape[0]
    wd = w.double().requires_grad_(True)
    ((wd * dW[:, :c].double()).sum() + ld_coef * torch.linalg.slogdet(wd)[1]).backward()
    _, _, inv, cond = _reference(w)
    ref = wd.grad + (g0.double().view(c, c) if accumulate else 0.0)
    tol = abs(ld_coef) * _inv_bound(c, cond, inv) + U32 * (2 * ref.abs() + 2 * wd.grad.abs() + g0.double().view(c, c).abs())
    err = (got.double().cpu().view(c, c) - ref).abs()
    assert bool((err <= tol).all()), (c, float((err / tol).max()))
    return float((err / tol).max())


@pytest.mark.parametrize('c', SIZES)
def test_invconv_plain_bwd(c):
    from mcgen_amd import ops
    ld_coef = -0.37 * 64
    jobs, checks = [], []
    for ldw in (c, c + 8):
        for accumulate in (0, 1):
            w, dW, g0 = _bwd_case(c, ldw, accumulate, 1000 * c + 10 * ldw + accumulate)
            _, winv = ops.invconv_plain(w.cuda())
            grad = g0.cuda().clone() if accumulate else torch.full((c, c, 1, 1), float('nan'), device='cuda')
            dWd = dW.cuda()
            ops.invconv_plain_bwd(dWd, winv, ld_coef, grad, bool(accumulate))
            worst = _bwd_check(w, dW, g0, accumulate, ld_coef, grad)
            print(f'C={c} ldw={ldw} accumulate={accumulate}: worst err / bound {worst:.3g}')
            # the log-determinant term is a real part of the result, not rounding noise
            assert float((grad.cpu().view(c, c) - dW[:, :c] - (g0.view(c, c) if accumulate else 0)).abs().max()) > 1.0
            again = g0.cuda().clone() if accumulate else torch.empty((c, c, 1, 1), device='cuda')
            jobs.append((dWd, winv, ld_coef, again, accumulate))
            checks.append(grad)
    ops.invconv_plain_bwd_batch(jobs)                                        # the batched form: the same bits
    for (_, _, _, again, _), grad in zip(jobs, checks):
        assert torch.equal(again, grad)


def test_invconv_plain_bwd_batch_over_the_launch_limit():
    from mcgen_amd import _lib, ops
    jobs, single = [], []
    for i in range(_lib.CONSTANTS['MCGEN_GLOW_BATCH_MAX'] + 5):
        c = SIZES[i % len(SIZES)]
        w, dW, g0 = _bwd_case(c, c + 8 * (i % 2), i % 2, 50 + i)
        _, winv = ops.invconv_plain(w.cuda())
        a, b = g0.cuda().clone(), g0.cuda().clone()
        ops.invconv_plain_bwd(dW.cuda(), winv, 0.5 + i, a, bool(i % 2))
        jobs.append((dW.cuda(), winv, 0.5 + i, b, i % 2)); single.append(a)
    ops.invconv_plain_bwd_batch(jobs)
    for j, a in zip(jobs, single):
        assert torch.equal(j[3], a)


# ---- additive coupling -----------------------------------------------------------------------------------------------------------
def _pad8(c):
    return (c + 7) // 8 * 8


def _coupling_inputs(c, cp, hw, dtype, seed, dyadic):
    """x [3, side, side, Cp] and h [3, side, side, pad8(C/2)], the pad channels of both filled too (they must be ignored).
    dyadic: multiples of 2^-10 below 4 in magnitude, so that every sum x + h is exact in fp32 (and in bf16 the inputs are
    exact)."""
    g = torch.Generator().manual_seed(seed)
    side = int(round(hw ** 0.5))
    shape_x, shape_h = (3, side, side, cp), (3, side, side, _pad8(c // 2))
    if dyadic:
        x = torch.randint(-4096, 4096, shape_x, generator=g).float() / 1024
        h = torch.randint(-4096, 4096, shape_h, generator=g).float() / 1024
    else:
        x, h = torch.randn(shape_x, generator=g), torch.randn(shape_h, generator=g)
    return x.to(dtype).cuda(), h.to(dtype).cuda()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('hw', [4, 16, 256])
@pytest.mark.parametrize('c,cp', [(4, 8), (12, 16), (16, 16), (48, 48)])
def test_coupling_add(c, cp, hw, dtype):
    from mcgen_amd import ops
    half = c // 2
    u = U32 if dtype == torch.float32 else UBF
    for dyadic in (False, True):
        x, h = _coupling_inputs(c, cp, hw, dtype, 31 * c + hw + dyadic, dyadic)
        for reverse in (False, True):
            y = torch.full_like(x, float('nan'))                              # garbage: every channel of y has to be written
            got = ops.glow_coupling_add(x, h, c, reverse=reverse, out=y)
            assert got is y
            ref = x[..., half:c].double() + (-1.0 if reverse else 1.0) * h[..., :half].double()
            err = (y[..., half:c].double() - ref).abs()
            # one rounding of the output dtype (bf16: of the fp32 sum, itself rounded once)
            assert bool((err <= u * ref.abs() + (U32 * ref.abs() if dtype != torch.float32 else 0.0)).all()), float(err.max())
            assert torch.equal(y[..., :half], x[..., :half])                  # the first half: the same bits
            if cp > c:
                assert float(y[..., c:].float().abs().max()) == 0.0
            z = x.clone()
            assert ops.glow_coupling_add(z, h, c, reverse=reverse, out=z) is z and torch.equal(z, y)      # in place
            assert torch.equal(ops.glow_coupling_add(x, h, c, reverse=reverse), y)
        if dyadic and dtype == torch.float32:
            # forward then reverse returns x exactly where x + h is representable, as it is for these inputs
            fwd = ops.glow_coupling_add(x, h, c)
            back = ops.glow_coupling_add(fwd, h, c, reverse=True)
            assert torch.equal(back[..., :c], x[..., :c])
            assert torch.equal(fwd[..., half:c], x[..., half:c] + h[..., :half])


def test_wrappers_refuse_bad_tensors():
    from mcgen_amd import _lib, ops
    w = _matrices(8, 1)[0][1].cuda()
    _, winv = ops.invconv_plain(w)
    grad = torch.zeros(8, 8, device='cuda')
    bad = [lambda: ops.invconv_plain(w.double()),                                           # wrong dtype
           lambda: ops.invconv_plain(w.bfloat16()),
           lambda: ops.invconv_plain(w.t()),                                                # not contiguous
           lambda: ops.invconv_plain(torch.eye(65, device='cuda')),                         # C > 64
           lambda: ops.invconv_plain(torch.zeros(8, 4, device='cuda')),                     # not square
           lambda: ops.invconv_plain(w.cpu()),                                              # no CPU path
           lambda: ops.invconv_plain_batch([w, torch.eye(65, device='cuda')]),
           lambda: ops.invconv_plain_batch([w, w.t()]),
           lambda: ops.invconv_plain_bwd(torch.zeros(8, 4, device='cuda'), winv, 1.0, grad),    # row pitch below C
           lambda: ops.invconv_plain_bwd(torch.zeros(8, 16, device='cuda')[:, :8], winv, 1.0, grad),   # not contiguous
           lambda: ops.invconv_plain_bwd(torch.zeros(8, 8, device='cuda'), winv.double(), 1.0, grad),
           lambda: ops.invconv_plain_bwd(torch.zeros(8, 8, device='cuda'), winv, 1.0, torch.zeros(8, 4, device='cuda')),
           lambda: ops.invconv_plain_bwd_batch([(torch.zeros(8, 8, device='cuda'), winv.t(), 1.0, grad, 0)])]
    x, h = _coupling_inputs(12, 16, 16, torch.float32, 3, False)
    bad += [lambda: ops.glow_coupling_add(x, h, 11),                                        # odd C
            lambda: ops.glow_coupling_add(x, h, 24),                                        # C above the pitch
            lambda: ops.glow_coupling_add(x, h.bfloat16(), 12),                             # dtypes differ
            lambda: ops.glow_coupling_add(x.half(), h.half(), 12),                          # no such compute dtype
            lambda: ops.glow_coupling_add(x, h[..., :4], 12),                               # h narrower than C / 2 (and strided)
            lambda: ops.glow_coupling_add(x[:, :, :2], h[:, :, :2], 12),                    # not contiguous
            lambda: ops.glow_coupling_add(x, h[:2], 12),                                    # other pixels
            lambda: ops.glow_coupling_add(x.cpu(), h.cpu(), 12)]
    for i, f in enumerate(bad):
        with pytest.raises(_lib.McgenError):
            f()
            pytest.fail(f'case {i} was not refused')
    torch.cuda.synchronize()
    assert float(grad.abs().max()) == 0.0                                                   # nothing was launched
