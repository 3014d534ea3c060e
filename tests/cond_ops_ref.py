"""Float64 CPU references for the label-conditioning kernels of the conditional baselines: csrc/cgan_ops.hip,
csrc/cvae_ops.hip, csrc/cpixelcnn_ops.hip and csrc/cglow_ops.hip.  They restate the formulas of the file headers and of the
reference's cgan.py, cvae.py, cpixelcnn.py and cglow.py, never the kernels' decompositions: the embedding input gradients
are autograd through a float64 F.conv2d of the broadcast embedding (no window sums, no border classes, no slices).

Every function takes the exact values a kernel read (bf16 inputs already rounded to bf16, fp32 scalars at their fp32
value) and returns float64 tensors.  Where a bound needs it a function also returns `mag`, the sum of the magnitudes of the
terms of each output (the same formula on absolute values: every such output is linear in its terms).
test_cond_ops_ref_cpu.py checks this file against torch autograd of the module formulas; test_cond_baseline_kernels_gpu.py
checks the kernels against it.  The CGlow prior itself lives in cglow_ref.py and is reused from there."""
import numpy as np
import torch
import torch.nn.functional as F

import cglow_ref
import pixel_ops_ref as P

F64 = torch.float64


def _d(*ts):
    return [None if t is None else torch.as_tensor(t).to(F64) for t in ts]


# ---- the embedding tables of CGAN, CVAE (w [E, M], column = mode) -------------------------------------------------------
def embed(w, label):
    """embedding(one_hot(label)) = w[:, label] -> [N, E]; a label outside [0, M) gives a zero row."""
    w, = _d(w)
    label = torch.as_tensor(label).long()
    ok = (label >= 0) & (label < w.shape[1])
    rows = w.t()[torch.where(ok, label, torch.zeros_like(label))]
    return torch.where(ok[:, None], rows, torch.zeros_like(rows))


def embed_bwd(de, label, m, base=None):
    """dW[:, k] = (base +) sum over the samples with label == k of de[n] -> (dW [E, M], mag); labels outside add nothing."""
    de, base = _d(de, base)
    label = torch.as_tensor(label).long()
    ok = (label >= 0) & (label < m)
    out = []
    for t in (de, de.abs()):
        dw = torch.zeros(m, de.shape[1], dtype=F64).index_add_(0, label[ok], t[ok]).t()
        out.append(dw)
    if base is not None:
        out[0], out[1] = out[0] + base, out[1] + base.abs()
    return out[0].contiguous(), out[1].contiguous()


def gen_input(z, w, label):
    """cat(z, w[:, label]) -> [N, L + E] (cgan.py:57-59, cvae.py:92-95)."""
    z, = _d(z)
    return torch.cat([z, embed(w, label)], 1)


def dis_input(img, w, sigma, label):
    """img [N, HW, Cimg] -> cat(img, (w / sigma)[:, label] at every pixel) [N, HW, Cimg + E] (cgan.py:166-169)."""
    img, = _d(img)
    e = embed(w, label) / float(sigma)
    return torch.cat([img, e[:, None, :].expand(-1, img.shape[1], -1)], 2)


def lin_dembed(dlin, w, col0, e):
    """The Linear's input gradient at columns [col0, col0 + E): dlin [N, 4, 4, C0] holds the gradient of output row
    c * 16 + p at [n, p, c]; w [16 C0, in_features] -> (dE [N, E], mag)."""
    dlin, w = _d(dlin, w)
    n, c0 = dlin.shape[0], dlin.shape[-1]
    dy = dlin.reshape(n, 16, c0).permute(0, 2, 1).reshape(n, 16 * c0)                # column c * 16 + p
    out = []
    for g, wt in ((dy, w), (dy.abs(), w.abs())):
        x = torch.zeros(n, w.shape[1], dtype=F64, requires_grad=True)
        (F.linear(x, wt) * g).sum().backward()
        out.append(x.grad[:, col0:col0 + e].clone())
    return out[0], out[1]


def _broadcast_grad(fn, n, e, h, w):
    """d/d emb of fn(x), x[n, :, i, j] = emb[n] at every pixel of an h x w map."""
    emb = torch.zeros(n, e, dtype=F64, requires_grad=True)
    fn(emb[:, :, None, None].expand(n, e, h, w)).backward()
    return emb.grad.clone()


def dis_dembed(dc1, dy, w1, wsc, sigma1, sigma_sc, cimg, e):
    """The discriminator embedding's input gradient through FirstDisResBlock: conv1 = 3x3 pad 1 with weight w1 / sigma1
    (output gradient dc1 [N, H, W, C]) plus the shortcut avg_pool2d(1x1(x), 2) with weight wsc / sigma_sc (output gradient
    dy [N, H/2, W/2, C]); w1 [C, Cin, 3, 3], wsc [C, Cin], the embedding at input channels [cimg, cimg + E) -> (dE, mag)."""
    dc1, dy, w1, wsc = _d(dc1, dy, w1, wsc)
    n, h, w, c = dc1.shape
    out = []
    for absval in (False, True):
        k1 = w1[:, cimg:cimg + e] / float(sigma1)
        ks = (wsc[:, cimg:cimg + e] / float(sigma_sc))[:, :, None, None]
        g1, g2 = dc1.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
        if absval:
            k1, ks, g1, g2 = k1.abs(), ks.abs(), g1.abs(), g2.abs()

        def fn(x):
            return (F.conv2d(x, k1, padding=1) * g1).sum() + (F.avg_pool2d(F.conv2d(x, ks), 2) * g2).sum()
        out.append(_broadcast_grad(fn, n, e, h, w))
    return out[0], out[1]


def enc_input(img, w, label):
    """img NCHW [N, C, H, W] in (-1, 1) -> cat((img + 1) / 2, w[:, label] at every pixel), NHWC [N, HW, C + E] (cvae.py:58-62)."""
    img, = _d(img)
    n, c = img.shape[:2]
    x = ((img + 1) / 2).reshape(n, c, -1).permute(0, 2, 1)
    return torch.cat([x, embed(w, label)[:, None, :].expand(-1, x.shape[1], -1)], 2)


def enc_dembed(d_h, w, cimg, e):
    """The encoder embedding's input gradient through Conv2d(Cin, C, 4, 2, 1): output gradient d_h [N, Ho, Wo, C],
    w [C, Cin, 4, 4] -> (dE [N, E], mag)."""
    d_h, w = _d(d_h, w)
    n, ho, wo, c = d_h.shape
    out = []
    for absval in (False, True):
        k, g = w[:, cimg:cimg + e], d_h.permute(0, 3, 1, 2)
        if absval:
            k, g = k.abs(), g.abs()
        out.append(_broadcast_grad(lambda x: (F.conv2d(x, k, stride=2, padding=1) * g).sum(), n, e, 2 * ho, 2 * wo))
    return out[0], out[1]


def latent_fwd(ml, eps, w, label):
    """ml [N, 2L] = mu | logvar -> dict: mu, logvar, z = mu + eps exp(logvar / 2) (or mu), zrow = cat(z, w[:, label]),
    kl [N] = 0.5 sum_j (mu^2 + exp(logvar) - 1 - logvar), kl_mag [N] = 0.5 sum_j (mu^2 + exp(logvar) + 1 + |logvar|),
    kld = sum_n kl (cvae.py:24-28, 127-131)."""
    ml, eps = _d(ml, eps)
    lat = ml.shape[1] // 2
    mu, lv = ml[:, :lat], ml[:, lat:]
    sd = torch.exp(0.5 * lv)
    z = mu if eps is None else mu + eps * sd
    kl = 0.5 * (mu * mu + torch.exp(lv) - 1 - lv).sum(1)
    return {'mu': mu, 'logvar': lv, 'z': z, 'noise': None if eps is None else eps * sd, 'zrow': torch.cat([z, embed(w, label)], 1),
            'kl': kl, 'kl_mag': 0.5 * (mu * mu + torch.exp(lv) + 1 + lv.abs()).sum(1), 'kld': kl.sum()}


def latent_bwd(dz, mu, logvar, eps, inv_numel):
    """The gradient of loss = f(z) + inv_numel * kld at (mu, logvar), given dz = df/dz [N, L]:
    dmu = dz + mu inv_numel, dlogvar = dz eps exp(logvar / 2) / 2 + (exp(logvar) - 1) inv_numel / 2
    -> dict with both, and the two terms of each."""
    dz, mu, lv, eps = _d(dz, mu, logvar, eps)
    a, b = dz * eps * 0.5 * torch.exp(0.5 * lv), 0.5 * (torch.exp(lv) - 1) * inv_numel
    return {'dmu': dz + mu * inv_numel, 'dmu_terms': (dz, mu * inv_numel), 'dlogvar': a + b, 'dlogvar_terms': (a, b),
            'exp_lv': torch.exp(lv)}


# ---- CGlow: the prior is cglow_ref's; only the magnitudes are added here ----------------------------------------------
def prior(b_p, s_p, w_e, b_e, s_e, label, hw):
    """cglow_ref.prior as a tensor, and its two terms' magnitudes [N, C2] -> (h [N, hw, C2], (|b_p rp|, |(e + b_e) re|))."""
    args = [np.asarray(torch.as_tensor(t).double()) for t in (b_p, s_p, w_e, b_e, s_e)]
    lab = np.asarray(torch.as_tensor(label))
    h = torch.from_numpy(cglow_ref.prior(*args, lab, hw))
    b_p, s_p, w_e, b_e, s_e = (torch.from_numpy(a) for a in args)
    t1 = (b_p * torch.exp(3 * s_p)).abs()[None].expand(len(lab), -1)
    t2 = ((embed(w_e, label) + b_e) * torch.exp(3 * s_e)).abs()
    return h, (t1, t2)


def prior_bwd(dprior, b_p, s_p, w_e, b_e, s_e, label):
    """cglow_ref.prior_bwd -> (grads, mags): dicts of float64 tensors keyed b_p, s_p, w_e, b_e, s_e, plus dh [N, C2];
    mags from the same formulas on |dprior|, |b_p|, |w_e|, |b_e|."""
    args = [np.asarray(torch.as_tensor(t).double()) for t in (dprior, b_p, s_p, w_e, b_e, s_e)]
    lab = np.asarray(torch.as_tensor(label))
    g = {k: torch.from_numpy(v) for k, v in cglow_ref.prior_bwd(*args, lab).items()}
    g['dh'] = torch.from_numpy(args[0].sum(1))
    a = [np.abs(args[0]), np.abs(args[1]), args[2], np.abs(args[3]), np.abs(args[4]), args[5]]
    m = {k: torch.from_numpy(v) for k, v in cglow_ref.prior_bwd(*a, lab).items()}
    m['dh'] = torch.from_numpy(a[0].sum(1))
    return g, m


# ---- CPixelCNN (table [M, 2C], row = mode; gathers clamp) ---------------------------------------------------------------
def cpx_rows(table, label):
    """table[clamp(label, 0, M - 1)] -> [N, 2C]."""
    table, = _d(table)
    return table[torch.as_tensor(label).long().clamp(0, table.shape[0] - 1)]


def cpx_gate_input(s, table, label):
    """s [N, HW, 2C] + the sample's row at every pixel: what both gates read (cpixelcnn.py:52, 56)."""
    s, = _d(s)
    return s + cpx_rows(table, label)[:, None, :]


def cpx_gated_fwd(s, table, label, scale, shift):
    """relu((a + e_a) scale + shift) * sigmoid(b + e_b) -> [N, HW, C]."""
    x = cpx_gate_input(s, table, label)
    return P.gated_fwd(x, scale, shift, torch.ones(x.shape[0], x.shape[-1] // 2, dtype=F64))


def cpx_gated_bwd_stats(s, table, label, scale, shift, mean, rstd, g):
    """pixel_ops_ref.gated_bwd_stats on s + e with code 1 -> (dz, db, s1, s2)."""
    x = cpx_gate_input(s, table, label)
    return P.gated_bwd_stats(x, scale, shift, mean, rstd, torch.ones(x.shape[0], x.shape[-1] // 2, dtype=F64), g)


def cpx_embed_bwd(dsum_v, dsum_h, label, m):
    """dE[k] = sum over the samples with label == k of dsum_v[n] + dsum_h[n] -> (dE [M, 2C], mag); a label outside [0, M)
    is skipped (not clamped)."""
    dsum_v, dsum_h = _d(dsum_v, dsum_h)
    label = torch.as_tensor(label).long()
    ok = (label >= 0) & (label < m)
    t = dsum_h if dsum_v is None else dsum_v + dsum_h
    ta = dsum_h.abs() if dsum_v is None else dsum_v.abs() + dsum_h.abs()
    z = torch.zeros(m, t.shape[1], dtype=F64)
    return z.clone().index_add_(0, label[ok], t[ok]), z.clone().index_add_(0, label[ok], ta[ok])


def cpx_gather_rows(tables, label):
    """tables [L, M, 2C] -> [L, N, 2C], labels clamped."""
    tables, = _d(tables)
    return tables[:, torch.as_tensor(label).long().clamp(0, tables.shape[1] - 1)]


def cpx_code_embed_bwd(dx, codes, k):
    """dE[j] = sum over the pixels with codes == j of dx[p] -> (dE [K, C], mag); dx [P, C]; codes outside [0, K) add nothing."""
    dx, = _d(dx)
    codes = torch.as_tensor(codes).long().reshape(-1)
    ok = (codes >= 0) & (codes < k)
    z = torch.zeros(k, dx.shape[1], dtype=F64)
    return z.clone().index_add_(0, codes[ok], dx[ok]), z.clone().index_add_(0, codes[ok], dx[ok].abs())
