"""tests/cond_ops_ref.py against torch float64 autograd of the module formulas of the reference's cgan.py, cvae.py,
cpixelcnn.py and cglow.py, at two or three small shapes each, and the edge semantics the kernels document: a label outside
[0, M) is a zero row without gradient for the CGAN, CVAE and CGlow tables, is clamped by CPixelCNN's gathers and skipped by
its table gradient; a code outside [0, K) adds nothing."""
import pytest
import torch
import torch.nn.functional as F

import cond_ops_ref as R
import pixel_ops_ref as P

F64 = torch.float64
TOL = 1e-12


def _close(a, b, what, tol=TOL):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max() / (b.abs().max() + 1e-300))
    assert err <= tol, (what, err)


def _mag_ok(val, mag, what):
    assert bool((mag >= val.abs() * (1 - 1e-12)).all()), what


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=F64)


@pytest.mark.parametrize('n,lat,e,m,c0', [(3, 5, 4, 6, 2), (2, 1, 1, 1, 1), (4, 7, 8, 3, 3)])
def test_cgan_generator_input_and_gradients(n, lat, e, m, c0):
    """Generator (cgan.py:56-60): x = cat(z, Linear(M, E, bias=False)(one_hot(label))) -> Linear(L + E, 16 C0)."""
    gen = _g(n + e)
    z, w_emb = _rn(gen, n, lat), _rn(gen, e, m).requires_grad_(True)
    w_lin, dy = _rn(gen, 16 * c0, lat + e + 2), _rn(gen, n, 16 * c0)
    label = torch.randint(0, m, (n,), generator=gen)
    emb = F.linear(F.one_hot(label, m).double(), w_emb)
    emb.retain_grad()
    x = torch.cat([z, emb, torch.zeros(n, 2, dtype=F64)], 1)
    (F.linear(x, w_lin) * dy).sum().backward()
    _close(R.gen_input(z, w_emb.detach(), label), x[:, :lat + e].detach(), 'gen_input')
    dlin = dy.reshape(n, c0, 16).permute(0, 2, 1).reshape(n, 4, 4, c0)            # [n, p, c] = d output row c * 16 + p
    de, mag = R.lin_dembed(dlin, w_lin, lat, e)
    _close(de, emb.grad, 'lin_dembed')
    _mag_ok(de, mag, 'lin_dembed mag')
    _close(R.lin_dembed(dlin.abs(), w_lin.abs(), lat, e)[0], R.lin_dembed(dlin.abs(), w_lin.abs(), lat, e)[1], 'mag = value on |.|')
    dw, dmag = R.embed_bwd(emb.grad, label, m)
    _close(dw, w_emb.grad, 'embed_bwd')
    _mag_ok(dw, dmag, 'embed_bwd mag')
    base = _rn(gen, e, m)
    _close(R.embed_bwd(emb.grad, label, m, base)[0], w_emb.grad + base, 'embed_bwd accumulate')


@pytest.mark.parametrize('n,h,w,c,cimg,e,m', [(2, 4, 6, 5, 3, 4, 3), (3, 2, 2, 2, 1, 1, 1), (2, 6, 4, 3, 0, 2, 4)])
def test_cgan_discriminator_input_and_gradient(n, h, w, c, cimg, e, m):
    """Discriminator (cgan.py:161-166) into FirstDisResBlock (cgan.py:102-122) with spectral-normalised weights w / sigma."""
    gen = _g(h * w + c)
    img, w_emb = _rn(gen, n, cimg, h, w), _rn(gen, e, m).requires_grad_(True)
    w1, wsc = _rn(gen, c, cimg + e + 1, 3, 3), _rn(gen, c, cimg + e + 1)
    s1, ssc, sig = 1.7, 0.6, 1.3
    dc1, dy = _rn(gen, n, c, h, w), _rn(gen, n, c, h // 2, w // 2)
    label = torch.randint(0, m, (n,), generator=gen)
    emb = F.linear(F.one_hot(label, m).double(), w_emb / sig)
    emb.retain_grad()
    x = torch.cat([img, emb[:, :, None, None].expand(n, e, h, w), torch.zeros(n, 1, h, w, dtype=F64)], 1)
    loss = (F.conv2d(x, w1 / s1, padding=1) * dc1).sum() + (F.avg_pool2d(F.conv2d(x, (wsc / ssc)[:, :, None, None]), 2) * dy).sum()
    loss.backward()
    got = R.dis_input(img.permute(0, 2, 3, 1).reshape(n, h * w, cimg), w_emb.detach(), sig, label)
    _close(got, x[:, :cimg + e].detach().permute(0, 2, 3, 1).reshape(n, h * w, cimg + e), 'dis_input')
    de, mag = R.dis_dembed(dc1.permute(0, 2, 3, 1), dy.permute(0, 2, 3, 1), w1, wsc, s1, ssc, cimg, e)
    _close(de, emb.grad, 'dis_dembed')
    _mag_ok(de, mag, 'dis_dembed mag')
    _close(R.embed_bwd(emb.grad / sig, label, m)[0], w_emb.grad, 'table gradient through 1 / sigma')


@pytest.mark.parametrize('n,ho,wo,c,cimg,e,m', [(2, 2, 3, 5, 3, 4, 3), (3, 1, 1, 2, 1, 1, 1), (2, 3, 2, 3, 2, 2, 4)])
def test_cvae_encoder_input_and_gradient(n, ho, wo, c, cimg, e, m):
    """Encoder (cvae.py:58-63): cat((img + 1) / 2, embedding) -> Conv2d(C + E, h0, 4, 2, 1)."""
    gen = _g(ho * wo + c)
    h, w = 2 * ho, 2 * wo
    img, w_emb = torch.rand(n, cimg, h, w, generator=gen, dtype=F64) * 2 - 1, _rn(gen, e, m).requires_grad_(True)
    wc, d_h = _rn(gen, c, cimg + e, 4, 4), _rn(gen, n, c, ho, wo)
    label = torch.randint(0, m, (n,), generator=gen)
    emb = F.linear(F.one_hot(label, m).double(), w_emb)
    emb.retain_grad()
    x = torch.cat([(img + 1) / 2, emb[:, :, None, None].expand(n, e, h, w)], 1)
    (F.conv2d(x, wc, stride=2, padding=1) * d_h).sum().backward()
    _close(R.enc_input(img, w_emb.detach(), label), x.detach().permute(0, 2, 3, 1).reshape(n, h * w, cimg + e), 'enc_input')
    de, mag = R.enc_dembed(d_h.permute(0, 2, 3, 1), wc, cimg, e)
    _close(de, emb.grad, 'enc_dembed')
    _mag_ok(de, mag, 'enc_dembed mag')
    _close(R.embed_bwd(emb.grad, label, m)[0], w_emb.grad, 'embed_bwd')


@pytest.mark.parametrize('n,lat,e,m', [(3, 5, 4, 3), (2, 1, 1, 1), (4, 9, 2, 5)])
def test_cvae_latent_step(n, lat, e, m):
    """reparameterize (cvae.py:53-56), the decoder's cat (cvae.py:94-95) and the KL term of loss (cvae.py:11)."""
    gen = _g(lat + e)
    mu, lv = _rn(gen, n, lat).requires_grad_(True), _rn(gen, n, lat).requires_grad_(True)
    eps, w_emb, dz = _rn(gen, n, lat), _rn(gen, e, m), _rn(gen, n, lat)
    label = torch.randint(0, m, (n,), generator=gen)
    inv = 1.0 / 37
    z = mu + eps * torch.exp(0.5 * lv)
    kld = 0.5 * torch.sum(mu.pow(2) + lv.exp() - 1 - lv)
    ((z * dz).sum() + inv * kld).backward()
    f = R.latent_fwd(torch.cat([mu, lv], 1).detach(), eps, w_emb, label)
    _close(f['zrow'], torch.cat([z.detach(), F.one_hot(label, m).double() @ w_emb.t()], 1), 'zrow')
    _close(f['kld'], kld.detach(), 'kld')
    _close(f['kl'].sum(), kld.detach(), 'kl per sample')
    _mag_ok(f['kl'], f['kl_mag'], 'kl mag')
    _close(R.latent_fwd(torch.cat([mu, lv], 1).detach(), None, w_emb, label)['z'], mu.detach(), 'evaluation: z = mu')
    b = R.latent_bwd(dz, mu.detach(), lv.detach(), eps, inv)
    _close(b['dmu'], mu.grad, 'dmu')
    _close(b['dlogvar'], lv.grad, 'dlogvar')
    _close(b['dmu_terms'][0] + b['dmu_terms'][1], mu.grad, 'dmu terms')
    _close(b['dlogvar_terms'][0] + b['dlogvar_terms'][1], lv.grad, 'dlogvar terms')
    big = torch.cat([mu.detach(), torch.full((n, lat), 800.0, dtype=F64)], 1)
    assert bool(torch.isinf(R.latent_fwd(big, eps, w_emb, label)['kl']).all())           # exp overflows to inf, not NaN


@pytest.mark.parametrize('n,hw,c2,m', [(3, 4, 6, 3), (2, 1, 2, 1)])
def test_cglow_prior_and_gradients(n, hw, c2, m):
    """Block.forward of the last block (cglow.py:231-235): ZeroConv2d(zeros) + ZeroConv2d(one_hot), ZeroConv2d(x) =
    (conv(x) + b) exp(3 scale)."""
    gen = _g(c2 + m)
    b_p, s_p, b_e, s_e = (_rn(gen, c2).requires_grad_(True) for _ in range(4))
    w_e, dprior = _rn(gen, c2, m).requires_grad_(True), _rn(gen, n, hw, c2)
    label = torch.randint(0, m, (n,), generator=gen)
    h = b_p * torch.exp(3 * s_p) + (F.one_hot(label, m).double() @ w_e.t() + b_e) * torch.exp(3 * s_e)
    (h[:, None, :] * dprior).sum().backward()
    args = [t.detach() for t in (b_p, s_p, w_e, b_e, s_e)]
    got, (t1, t2) = R.prior(*args, label, hw)
    _close(got, h.detach()[:, None, :].expand(n, hw, c2), 'prior')
    _mag_ok(got[:, 0], t1 + t2, 'prior terms')
    g, mag = R.prior_bwd(dprior, *args, label)
    for k, p in (('b_p', b_p), ('s_p', s_p), ('w_e', w_e), ('b_e', b_e), ('s_e', s_e)):
        _close(g[k], p.grad, k)
        _mag_ok(g[k], mag[k], k + ' mag')
    _close(g['dh'], dprior.sum(1), 'dh')


@pytest.mark.parametrize('n,hw,c,m', [(3, 5, 4, 3), (2, 1, 2, 1), (4, 6, 8, 7)])
def test_cpixelcnn_conditional_gate(n, hw, c, m):
    """ConditionalGatedMaskedConv2d's gate (cpixelcnn.py:14-18, 52, 56): GatedActivation(s + Embedding(M, 2C)(label)) with a
    training-mode BatchNorm2d on the first half."""
    gen = _g(hw + c)
    s, table = _rn(gen, n, hw, 2 * c).requires_grad_(True), _rn(gen, m, 2 * c).requires_grad_(True)
    gamma, beta, g = _rn(gen, c).requires_grad_(True), _rn(gen, c).requires_grad_(True), _rn(gen, n, hw, c)
    label = torch.randint(0, m, (n,), generator=gen)
    x = s + F.embedding(label, table)[:, None, :]
    a, b = x[..., :c], x[..., c:]
    mean, var = a.mean((0, 1)), a.var((0, 1), unbiased=False)
    rstd = 1 / torch.sqrt(var + 1e-5)
    out = torch.relu((a - mean) * rstd * gamma + beta) * torch.sigmoid(b)
    (out * g).sum().backward()
    sc, sh = (gamma * rstd).detach(), (beta - mean * gamma * rstd).detach()
    sd, td, md, rd = s.detach(), table.detach(), mean.detach(), rstd.detach()
    xin = R.cpx_gate_input(sd, td, label)
    _close(xin[..., :c].reshape(-1, c).mean(0), md, 'statistics input')
    _close(R.cpx_gated_fwd(sd, td, label, sc, sh), out.detach(), 'cpx_gated_fwd')
    dz, db, s1, s2 = R.cpx_gated_bwd_stats(sd, td, label, sc, sh, md, rd, g)
    da = P.bn_apply(dz, xin[..., :c], sc, md, rd, s1, s2, n * hw)
    ds = torch.cat([da, db], -1)
    _close(ds, s.grad, 'ds', 1e-10)
    _close(s1, beta.grad, 'dbeta', 1e-10)
    _close(s2, gamma.grad, 'dgamma', 1e-10)
    de, mag = R.cpx_embed_bwd(None, ds.sum(1), label, m)
    _close(de, table.grad, 'cpx_embed_bwd', 1e-10)
    _mag_ok(de, mag, 'cpx_embed_bwd mag')
    _close(R.cpx_embed_bwd(ds.sum(1), ds.sum(1), label, m)[0], 2 * table.grad, 'two gates', 1e-10)
    tables = torch.stack([td, -td])
    _close(R.cpx_gather_rows(tables, label), torch.stack([td[label], -td[label]]), 'cpx_gather_rows')


@pytest.mark.parametrize('p,c,k', [(7, 3, 4), (1, 1, 1), (300, 5, 9)])
def test_cpixelcnn_code_embedding_gradient(p, c, k):
    """The input embedding nn.Embedding(K, C) of the code map (cpixelcnn.py:86-90)."""
    gen = _g(p + c)
    emb, dx = _rn(gen, k, c).requires_grad_(True), _rn(gen, p, c)
    codes = torch.randint(0, k, (p,), generator=gen)
    (F.embedding(codes, emb) * dx).sum().backward()
    de, mag = R.cpx_code_embed_bwd(dx, codes, k)
    _close(de, emb.grad, 'cpx_code_embed_bwd')
    _mag_ok(de, mag, 'mag')


def test_labels_and_codes_outside_their_range():
    gen = _g(9)
    e, m, n = 3, 4, 6
    w = _rn(gen, e, m)
    label = torch.tensor([-1, 0, m, m - 1, 2 ** 40, 2])
    ok = torch.tensor([False, True, False, True, False, True])
    # CGAN, CVAE, CGlow: a zero row and no gradient
    rows = R.embed(w, label)
    assert bool((rows[~ok] == 0).all())
    _close(rows[ok], w.t()[label[ok]], 'rows inside')
    z = _rn(gen, n, 2)
    assert bool((R.gen_input(z, w, label)[~ok, 2:] == 0).all())
    assert bool((R.dis_input(_rn(gen, n, 5, 1), w, 2.0, label)[~ok][:, :, 1:] == 0).all())
    assert bool((R.enc_input(_rn(gen, n, 1, 2, 2), w, label)[~ok][:, :, 1:] == 0).all())
    assert bool((R.latent_fwd(_rn(gen, n, 4), None, w, label)['zrow'][~ok, 2:] == 0).all())
    de = _rn(gen, n, e)
    _close(R.embed_bwd(de, label, m)[0], R.embed_bwd(de[ok], label[ok], m)[0], 'embed_bwd skips labels outside')
    vec = [_rn(gen, e) for _ in range(4)]
    args = (vec[0], vec[1], w, vec[2], vec[3])
    h = R.prior(*args, label, 2)[0]
    _close(h[~ok][:, 0], (vec[0] * torch.exp(3 * vec[1]) + vec[2] * torch.exp(3 * vec[3]))[None].expand(3, e), 'prior without a row')
    dp = _rn(gen, n, 2, e)
    g = R.prior_bwd(dp, *args, label)[0]
    _close(g['w_e'], R.prior_bwd(dp[ok], *args, label[ok])[0]['w_e'], 'prior_bwd skips labels outside')
    _close(g['b_e'], dp.sum((0, 1)) * torch.exp(3 * vec[3]), 'the bias still sees every sample')
    # CPixelCNN: gathers clamp, the table gradient skips
    table = _rn(gen, m, 2 * e)
    clamped = torch.tensor([0, 0, m - 1, m - 1, m - 1, 2])
    _close(R.cpx_rows(table, label), table[clamped], 'cpx_rows clamps')
    _close(R.cpx_gather_rows(table[None], label), table[None][:, clamped], 'cpx_gather_rows clamps')
    s = _rn(gen, n, 3, 2 * e)
    _close(R.cpx_gate_input(s, table, label), s + table[clamped][:, None, :], 'gate input clamps')
    dsum = _rn(gen, n, 2 * e)
    _close(R.cpx_embed_bwd(None, dsum, label, m)[0], R.cpx_embed_bwd(None, dsum[ok], label[ok], m)[0], 'cpx_embed_bwd skips')
    # codes outside [0, K) add nothing
    codes = torch.tensor([-1, 0, 5, 4, 10 ** 9, 2])
    dx = _rn(gen, n, 3)
    keep = (codes >= 0) & (codes < 5)
    _close(R.cpx_code_embed_bwd(dx, codes, 5)[0], R.cpx_code_embed_bwd(dx[keep], codes[keep], 5)[0], 'codes outside')
