"""The float64 references of tests/small_ops_ref.py against torch's own modules in float64 on the CPU:
torch.nn.utils.spectral_norm (power iteration, sigma, the weight gradient), torch.optim.Adam and F.batch_norm."""
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
