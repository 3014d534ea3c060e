"""The float64 references of tests/small_ops_ref.py against torch's own modules in float64 on the CPU:
torch.nn.utils.spectral_norm (power iteration, sigma, the weight gradient), torch.optim.Adam and F.batch_norm; the tail,
hinge, code and layout references against autograd, F.one_hot and F.avg_pool2d.  The last tests check the input conditions
of test_mcgan_tail_code_ops_gpu.py from the reference alone: its dyadic cases are exact in fp32 in any summation order and
its random fused-tail cases have no sample within four logit bounds of a hinge point."""
import pytest
import torch
import torch.nn.functional as F

import small_ops_ref as R

F64 = torch.float64


@pytest.mark.parametrize('shape', [(1, 5), (7, 3), (16, 3, 3, 3), (24, 16, 1, 1)])
def test_power_iteration_and_grad_fix_match_spectral_norm(shape):
    """One training forward of a float64 spectral-normed layer advances u, v as power_round does and scales the weight by
    1 / sigma; the gradient of the normalised weight taken back to weight_orig is grad_fix's."""
    gen = torch.Generator().manual_seed(sum(shape))
    lin = torch.nn.Linear(shape[1], shape[0]) if len(shape) == 2 else torch.nn.Conv2d(shape[1], shape[0], shape[2])
    lin = lin.double()
    with torch.no_grad():
        lin.weight.copy_(torch.randn(shape, generator=gen, dtype=F64))
    m = torch.nn.utils.spectral_norm(lin)
    m.train()
    rows = shape[0]
    w = m.weight_orig.detach().reshape(rows, -1).clone()
    u0 = m.weight_u.detach().clone()
    x = torch.randn(2, *shape[1:2], *([4, 4] if len(shape) == 4 else []), generator=gen, dtype=F64)
    m(x)
    u, v, sigma = R.power_round(w, u0)
    torch.testing.assert_close(m.weight_u.detach(), u, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(m.weight_v.detach(), v, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(m.weight.detach().reshape(rows, -1), w / sigma, rtol=1e-12, atol=1e-13)
    assert abs(R.sigma_eval(w, u, v) - sigma) <= 1e-12 * sigma
    gw = torch.randn(shape, generator=gen, dtype=F64)
    m.zero_grad()
    (m.weight * gw).sum().backward()
    ref = R.grad_fix(gw.reshape(rows, -1), w, u, v, sigma)
    torch.testing.assert_close(m.weight_orig.grad.reshape(rows, -1), ref, rtol=1e-10, atol=1e-12)


def test_power_iteration_exact_cases():
    """rows = 1: sigma = |w|.  Rank one W = a b^T: sigma = |a| |b|, u, v = +-a / |a|, +-b / |b|."""
    w = torch.tensor([[3.0, -4.0, 12.0]], dtype=F64)
    u, v, sigma = R.power_round(w, torch.tensor([-0.5], dtype=F64))
    assert sigma == pytest.approx(13.0, rel=1e-15) and float(u) == pytest.approx(-1.0)
    a, b = torch.tensor([1.0, -2.0, 2.0], dtype=F64), torch.tensor([3.0, 4.0], dtype=F64)
    u, v, sigma = R.power_round(torch.outer(a, b), torch.tensor([0.1, 0.2, 0.3], dtype=F64))
    assert sigma == pytest.approx(15.0, rel=1e-15)
    torch.testing.assert_close(u, a / 3.0 * torch.sign(u[0] / a[0]))
    torch.testing.assert_close(v, b / 5.0 * torch.sign(v[0] / b[0]))


@pytest.mark.parametrize('wd', [0.0, 0.25])
def test_adam_matches_torch_optim(wd):
    """Five steps of adam() against torch.optim.Adam in float64, weight decay included; then from t = 1000 on."""
    gen = torch.Generator().manual_seed(7)
    p = torch.randn(300, generator=gen, dtype=F64).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=2e-3, betas=(0.5, 0.999), eps=1e-8, weight_decay=wd)
    q, m, v = p.detach().clone(), torch.zeros(300, dtype=F64), torch.zeros(300, dtype=F64)
    for t in range(1, 6):
        g = torch.randn(300, generator=gen, dtype=F64)
        g[:10] = 0.0
        p.grad = g.clone()
        opt.step()
        q, m, v = R.adam(q, g, m, v, t, 2e-3, 0.5, 0.999, 1e-8, wd)
        torch.testing.assert_close(p.detach(), q, rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(opt.state[p]['exp_avg'], m, rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(opt.state[p]['exp_avg_sq'], v, rtol=1e-13, atol=1e-15)
    opt.state[p]['step'] = torch.tensor(999.0, dtype=F64)
    g = torch.randn(300, generator=gen, dtype=F64)
    p.grad = g.clone()
    opt.step()
    q, m, v = R.adam(q, g, m, v, 1000, 2e-3, 0.5, 0.999, 1e-8, wd)
    torch.testing.assert_close(p.detach(), q, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize('const', [False, True])
def test_batchnorm_references_match_f_batch_norm(const):
    """bn_stats / bn_running against F.batch_norm's training forward (two successive batches: momentum 0.3), bn_eval_affine
    against its evaluation forward, bn_backward against autograd; a constant channel (variance 0) included."""
    gen = torch.Generator().manual_seed(11)
    n, c, h = 3, 5, 4
    gamma = torch.randn(c, generator=gen, dtype=F64).requires_grad_(True)
    beta = torch.randn(c, generator=gen, dtype=F64).requires_grad_(True)
    rm, rv = torch.randn(c, generator=gen, dtype=F64), torch.rand(c, generator=gen, dtype=F64) + 0.5
    rm_t, rv_t = rm.clone(), rv.clone()
    means, unbs = [], []
    for k in range(2):
        x = (torch.randn(n, c, h, h, generator=gen, dtype=F64) * 2 + 1)
        if const:
            x[:, 0] = 0.75
        x.requires_grad_(True)
        y = F.batch_norm(x, rm_t, rv_t, gamma, beta, True, 0.3, 1e-5)
        xs = x.detach().permute(0, 2, 3, 1).reshape(-1, c)
        st = R.bn_stats(xs.sum(0), (xs * xs).sum(0), xs.shape[0], gamma.detach(), beta.detach(), 1e-5)
        torch.testing.assert_close(x.detach() * st['scale'].view(1, c, 1, 1) + st['shift'].view(1, c, 1, 1), y.detach(),
                                   rtol=1e-12, atol=1e-12)
        means.append(st['mean']); unbs.append(st['unb'])
        dz = torch.randn(n, c, h, h, generator=gen, dtype=F64)
        add = torch.randn(n, c, h, h, generator=gen, dtype=F64)
        gamma.grad = beta.grad = None
        y.backward(dz)
        dzs = dz.permute(0, 2, 3, 1).reshape(-1, c)
        xh = (xs - st['mean']) * st['rstd']
        s1, s2 = dzs.sum(0), (dzs * xh).sum(0)
        dx = R.bn_backward(dzs, xs, xs.shape[0], st['scale'], st['mean'], st['rstd'], s1, s2, add=add.permute(0, 2, 3, 1).reshape(-1, c))
        torch.testing.assert_close(dx, x.grad.permute(0, 2, 3, 1).reshape(-1, c) + add.permute(0, 2, 3, 1).reshape(-1, c),
                                   rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(s1, beta.grad, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(s2, gamma.grad, rtol=1e-10, atol=1e-12)
    erm, erv = R.bn_running(rm, rv, torch.stack(means), torch.stack(unbs), 0.3)
    torch.testing.assert_close(erm, rm_t, rtol=1e-13, atol=1e-14)
    torch.testing.assert_close(erv, rv_t, rtol=1e-13, atol=1e-14)
    x = torch.randn(n, c, h, h, generator=gen, dtype=F64)
    y = F.batch_norm(x, rm_t, rv_t, gamma.detach(), beta.detach(), False, 0.3, 1e-5)
    sc, sh = R.bn_eval_affine(gamma.detach(), beta.detach(), rm_t, rv_t, 1e-5)
    torch.testing.assert_close(x * sc.view(1, c, 1, 1) + sh.view(1, c, 1, 1), y, rtol=1e-12, atol=1e-12)


def test_colsum_reference():
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 5, 24, generator=gen, dtype=F64)
    torch.testing.assert_close(R.colsum(x, 16, alpha=0.5), 0.5 * x.sum((0, 1))[:16])
    got = R.colsum(x, 16, row_perm=16)        # the generator's linear bias: [16 positions x C] -> [C x 16 positions]
    torch.testing.assert_close(got, x.sum((0, 1))[:16])
    s = x.sum((0, 1))[:16]
    torch.testing.assert_close(R.colsum(x, 16, row_perm=2), s.view(2, 8).t().reshape(-1))


# ---- the tail, hinge, code and layout references -------------------------------------------------------------------------
@pytest.mark.parametrize('with_code', [False, True])
@pytest.mark.parametrize('mode', ['d_pair', 'g'])
def test_tail_and_hinge_references_match_autograd(mode, with_code):
    """relu -> * code -> sum -> F.linear(w / sigma, b) -> a hinge loss, differentiated by autograd in float64: the logits,
    the pooled features, d loss / d logit, d loss / d x, and the gradients of the normalised weight and the bias.  x holds
    exact zeros of both signs (relu's gradient there is 0) and logits exactly at the hinge points."""
    n, c, hw = 6, 24, 5
    t = R.tail_inputs(n, c, hw, False, with_code, 'cpu', mode)
    x = t['x'].double().requires_grad_(True)
    code = None if t['code'] is None else t['code'].double()
    sigma, b0 = float(t['sigma']), float(t['b'])
    wn = (t['w'].double() / sigma).requires_grad_(True)
    b = torch.tensor([b0], dtype=F64, requires_grad=True)
    pooled = torch.relu(x)
    pooled = (pooled if code is None else pooled * code.view(n, 1, c)).sum(1)
    pooled.retain_grad()
    logit = F.linear(pooled, wn.view(1, c), b).view(-1)
    ref = R.dtail(t['x'], t['code'], t['w'], b0, sigma)
    torch.testing.assert_close(ref['pooled'], pooled.detach(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(ref['logit'], logit.detach(), rtol=1e-13, atol=1e-13)
    assert bool((ref['pooled_abs'] >= ref['pooled'].abs()).all()) and bool((ref['logit_abs'] >= ref['logit'].abs() - 1e-12).all())
    # move two logits onto the hinge points exactly: the loss sees shifted logits, its gradient there must be 0
    shift = torch.zeros(n, dtype=F64)
    shift[0] = 1.0 - float(logit.detach()[0])
    shift[n - 1] = -1.0 - float(logit.detach()[n - 1])
    lg = logit + shift
    if mode == 'd_pair':
        loss = torch.relu(1 - lg[:n // 2]).mean() + torch.relu(1 + lg[n // 2:]).mean()
        rl, dr, df, la = R.hinge_d(lg.detach()[:n // 2], lg.detach()[n // 2:])
        dl = torch.cat([dr, df])
        assert float(dl[0]) == 0.0 and float(dl[n - 1]) == 0.0 and float(la) == float(rl)
    else:
        loss = -lg.mean()
        rl, dl, la = R.hinge_g(lg.detach())
        assert float(la) >= abs(float(rl))
    loss.backward()
    assert float(rl) == pytest.approx(float(loss), rel=1e-14)
    dx, mask = R.dtail_dx(dl, t['x'], t['code'], t['w'], sigma)
    torch.testing.assert_close(dx, x.grad, rtol=1e-13, atol=1e-15)
    assert bool((dx[~mask] == 0).all()) and not bool(mask[t['x'] == 0].any())
    dw, db, dwa, dba = R.dtail_wgrad(dl, ref['pooled'])
    torch.testing.assert_close(dw, wn.grad, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(db.view(1), b.grad, rtol=1e-12, atol=1e-14)
    assert bool((dwa >= dw.abs() - 1e-14).all()) and float(dba) >= abs(float(db)) - 1e-14
    (f1, f2) = R.dtail_pair_wgrad(dl, ref['pooled'], 1.25)
    a1 = R.dtail_wgrad(dl[:n // 2], ref['pooled'][:n // 2])
    a2 = R.dtail_wgrad(dl[n // 2:], ref['pooled'][n // 2:])
    torch.testing.assert_close(f1[0], a1[0]); torch.testing.assert_close(f2[0], a2[0] / 1.25)
    torch.testing.assert_close(f1[0] + 1.25 * f2[0], dw, rtol=1e-12, atol=1e-14)
    assert float(f1[1]) == float(a1[1]) and float(f2[1]) == float(a2[1])


def test_tanh_code_pool_and_rounding_references():
    gen = torch.Generator().manual_seed(5)
    z = torch.randn(50, generator=gen, dtype=F64).requires_grad_(True)
    dy = torch.randn(50, generator=gen, dtype=F64)
    y = torch.tanh(z)
    y.backward(dy)
    torch.testing.assert_close(R.tanh_bwd(dy, y.detach()), z.grad, rtol=1e-13, atol=1e-15)
    # indicator @ codebook: F.one_hot picks the row; n_half / scale touch the second half only
    cb = torch.randn(33, 12, generator=gen)
    label = torch.randint(0, 33, (10,), generator=gen)
    code = R.mc_code(F.one_hot(label, 33).float(), cb)
    assert torch.equal(code, cb[label].double())
    sc = R.mc_code(F.one_hot(label, 33).float(), cb, n_half=4, scale=R.f32(1.3))
    assert torch.equal(sc[:4], code[:4]) and torch.equal(sc[4:], code[4:] * R.f32(1.3))
    soft = torch.rand(10, 33, generator=gen)
    torch.testing.assert_close(R.mc_code(soft, cb), soft.double() @ cb.double())
    # 2x2 sums: the average pool times 4
    x = torch.randn(2, 6, 10, 8, generator=gen)
    s, sa = R.pool2_sum(x)
    torch.testing.assert_close(s, F.avg_pool2d(x.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) * 4, rtol=1e-14, atol=1e-14)
    assert bool((sa >= s.abs()).all())
    # round to nearest even to bf16: ties, both signs, against torch's conversion
    v = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -1 - 2.0 ** -8, -1 - 3 * 2.0 ** -8, 0.0, -0.0, 3.0e38])
    want = torch.tensor([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -1.0, -1 - 2.0 ** -6, 0.0, 0.0, float(torch.tensor(3.0e38).bfloat16())], dtype=F64)
    assert torch.equal(R.round_bf16(v.double()), want)
    r = torch.randn(4096, generator=gen)
    assert torch.equal(R.round_bf16(r.double()), r.bfloat16().double())


def test_cmap_record_and_affine_rows():
    """cmap_record on a hand-written row; mc_affine_rows against a dense gather."""
    row = torch.zeros(40)
    row[[1, 5, 31, 32, 39]] = torch.tensor([1.0, -2.0, 0.5, 3.0, 1.5])
    row[7] = -0.0
    cpos, cidx, cpre = R.cmap_record(row)
    assert cpos.tolist() == [-1, 0, -1, -1, -1, 1] + [-1] * 25 + [2, 3] + [-1] * 6 + [4]
    assert cidx.tolist() == [1, 5, 31, 32, 39] + [40] * 67 and cpre.tolist() == [0, 3, 5]
    gen = torch.Generator().manual_seed(9)
    code = (torch.rand(6, 16, generator=gen) < 0.5).float() * (1 + torch.rand(6, 16, generator=gen))
    code[0] = 0
    scale, shift = torch.randn(2, 16, generator=gen), torch.randn(2, 16, generator=gen)
    so, ho = R.mc_affine_rows(code, 24, scale, shift, group_n=3)
    for i in range(6):
        act = code[i].nonzero().flatten()
        assert torch.equal(so[i, :len(act)], scale[i // 3, act].double() * code[i, act].double())
        assert torch.equal(ho[i, :len(act)], shift[i // 3, act].double() * code[i, act].double())
        assert bool((so[i, len(act):] == 0).all()) and bool((ho[i, len(act):] == 0).all())
    so, ho = R.mc_affine_rows(code, 8)
    assert torch.equal(so[1], torch.cat([code[1][code[1] != 0].double(), torch.zeros(16, dtype=F64)])[:8]) and not bool(ho.any())


# ---- the input conditions of test_mcgan_tail_code_ops_gpu.py ---------------------------------------------------------------
@pytest.mark.parametrize('with_code', [False, True])
@pytest.mark.parametrize('shape', R.TAIL_EXACT_SHAPES)
def test_exact_tail_cases_are_exact_in_fp32(shape, with_code):
    """Every partial sum of the dyadic fused-tail cases fits fp32 (and x fits bf16), and the constructed samples sit where
    the test says: logits +1, -1, 0 in both halves."""
    t = R.tail_exact_inputs(*shape, with_code=with_code)
    R.assert_exact(R.tail_exact_bits(t), f'tail {shape}')
    assert torch.equal(t['x'].bfloat16().float(), t['x'])
    ref = R.dtail(t['x'], t['code'], t['w'], t['b'], t['sigma'])
    h = shape[0] // 2
    assert ref['logit'][[0, 1, 2, h, h + 1, h + 2]].tolist() == [1.0, -1.0, 0.0, 1.0, -1.0, 0.0]
    assert torch.equal(ref['logit'].float().double(), ref['logit']) and torch.equal(ref['pooled'].float().double(), ref['pooled'])


def test_exact_pool_case_is_exact():
    x = R.pool_exact_input(3, 4, 10, 24, 1)
    s, sa = R.pool2_sum(x)
    R.assert_exact(R.sum_bits(float(sa.max()), R.quantum(x)), 'pool2_sum')
    assert R.sum_bits(float(sa.max()), R.quantum(x)) <= 8 and torch.equal(R.round_bf16(s), s)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('with_code', [False, True])
@pytest.mark.parametrize('shape', R.FUSED_RANDOM)
def test_random_fused_tail_cases_have_no_undecided_sample(shape, with_code, bf16):
    """No reference logit of a random fused-tail case lies within 4 logit bounds of its hinge point, so the kernel's
    d loss / d logit is decided by the reference."""
    t = R.fused_inputs(*shape, bf16, with_code)
    ref = R.dtail(t['x'], t['code'], t['w'], t['b'], t['sigma'])
    _, tol_l = R.tail_bounds(t, ref)
    assert not bool(R.undecided(ref, tol_l, 'd_pair').any()), (shape, ref['logit'], tol_l)
