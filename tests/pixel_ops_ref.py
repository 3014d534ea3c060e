"""Float64 CPU references for the kernels of csrc/pixelcnn_ops.hip and csrc/vq_ops.hip (MCPixelCNN, CPixelCNN, MCVAE,
CVAE, VQ-VAE and the classifier): im2col / col2im, the gated activation and its backward, the BatchNorm -> code ->
residual tails and their backward, max-pooling, BCE with logits, cross-entropy, arg-min, the VQ training step and the
tanh + MSE loss.  Everything is NHWC.  Each function takes the exact values a kernel read (bf16 inputs already rounded to
bf16, fp32 scalars passed as their fp32 value, see f32) and returns float64 tensors; test_pixel_ops_ref_cpu.py checks
them against torch's own operators, test_pixel_vq_kernels_gpu.py checks the kernels against them."""
import torch

F64 = torch.float64


def f32(x: float) -> float:
    """The fp32 value a kernel receives for the Python float x."""
    return float(torch.tensor(x, dtype=torch.float32))


def _d(*ts):
    return [None if t is None else t.to(F64) for t in ts]


def _per_image(code, x):
    """code [N, C] broadcast over the pixel dimensions of x [N, ..., C]."""
    return code.reshape(code.shape[0], *([1] * (x.dim() - 2)), code.shape[1])


# ---- im2col / col2im ------------------------------------------------------------------------------------------------
def activate(x, scale=None, shift=None, relu=False, code=None):
    """The im2col prologue relu?(x * scale + shift) * code on [N, H, W, Cp]; code is [N, Cp]."""
    x, scale, shift, code = _d(x, scale, shift, code)
    if scale is not None:
        x = x * scale + shift
    if relu:
        x = x.clamp_min(0.0)
    if code is not None:
        x = x * _per_image(code, x)
    return x


def im2col(x, kh, kw, oh, ow, stride=1, scale=None, shift=None, relu=False, code=None):
    """col[n, ho, wo, i * kw + j, c] = X[n, ho * stride + i - oh, wo * stride + j - ow, c], 0 outside the map, where X is x
    after the prologue (zero padding applies to the activated tensor) -> [N, H / stride, W / stride, kh * kw * Cp]."""
    x = activate(x, scale, shift, relu, code)
    n, h, w, cp = x.shape
    ho, wo = h // stride, w // stride
    xp = torch.zeros(n, h + oh + kh, w + ow + kw, cp, dtype=F64)
    xp[:, oh:oh + h, ow:ow + w] = x
    col = torch.zeros(n, ho, wo, kh * kw, cp, dtype=F64)
    for i in range(kh):
        for j in range(kw):
            col[:, :, :, i * kw + j] = xp[:, i:i + ho * stride:stride, j:j + wo * stride:stride]
    return col.reshape(n, ho, wo, kh * kw * cp)


def col2im(dcol, cp, kh, kw, oh, ow, stride=1, bias=None, base=None):
    """The exact adjoint of im2col: [N, Ho, Wo, kh * kw * cp] -> [N, Ho * stride, Wo * stride, cp].  Starts from `base`
    (accumulate) or from `bias` on the channels < len(bias) and 0 on the rest."""
    dcol, bias, base = _d(dcol, bias, base)
    n, ho, wo, _ = dcol.shape
    h, w = ho * stride, wo * stride
    dcol = dcol.reshape(n, ho, wo, kh * kw, cp)
    dxp = torch.zeros(n, h + oh + kh, w + ow + kw, cp, dtype=F64)
    for i in range(kh):
        for j in range(kw):
            dxp[:, i:i + h:stride, j:j + w:stride] += dcol[:, :, :, i * kw + j]
    dx = dxp[:, oh:oh + h, ow:ow + w].clone()
    if base is not None:
        return dx + base
    if bias is not None:
        dx[..., :bias.numel()] += bias
    return dx


# ---- MCGatedActivation ----------------------------------------------------------------------------------------------
def gated_fwd(s, scale, shift, code):
    """s = [a | b] on [N, ..., 2C], code [N, C] -> code * relu(a * scale + shift) * sigmoid(b)."""
    s, scale, shift, code = _d(s, scale, shift, code)
    c = s.shape[-1] // 2
    a, b = s[..., :c], s[..., c:]
    return _per_image(code, a) * (a * scale + shift).clamp_min(0.0) * torch.sigmoid(b)


def gated_bwd_stats(s, scale, shift, mean, rstd, code, g):
    """First pass of the backward of gated_fwd -> (dz, db, s1, s2): dz = g code q [z > 0], db = g code relu(z) q (1 - q)
    with z = a scale + shift, q = sigmoid(b); s1 = sum dz, s2 = sum dz xhat over all pixels, xhat = (a - mean) rstd."""
    s, scale, shift, mean, rstd, code, g = _d(s, scale, shift, mean, rstd, code, g)
    c = s.shape[-1] // 2
    a, b = s[..., :c], s[..., c:]
    z = a * scale + shift
    q = torch.sigmoid(b)
    gk = g * _per_image(code, a)
    dz = torch.where(z > 0, gk * q, torch.zeros_like(z))
    db = gk * z.clamp_min(0.0) * q * (1 - q)
    xh = (a - mean) * rstd
    return dz, db, dz.reshape(-1, c).sum(0), (dz * xh).reshape(-1, c).sum(0)


def bn_apply(dz, x, scale, mean, rstd, s1, s2, count):
    """Second pass of a BatchNorm backward: scale (dz - (s1 + xhat s2) / count), scale = gamma rstd."""
    dz, x, scale, mean, rstd, s1, s2 = _d(dz, x, scale, mean, rstd, s1, s2)
    xh = (x - mean) * rstd
    return scale * (dz - (s1 + xh * s2) / count)


def gated_bwd(s, scale, shift, mean, rstd, code, g, round_dz=None):
    """Backward of gated_fwd through the batch statistics -> (ds [.., 2C], dgamma, dbeta).  round_dz, if given, is applied
    to dz between the passes (the kernels store dz in the compute dtype and read it back)."""
    c = s.shape[-1] // 2
    dz, db, s1, s2 = gated_bwd_stats(s, scale, shift, mean, rstd, code, g)
    if round_dz is not None:
        dz = round_dz(dz)
    count = dz.numel() // c
    da = bn_apply(dz, s[..., :c], scale, mean, rstd, s1, s2, count)
    return torch.cat([da, db], -1), s2, s1


# ---- BatchNorm -> code -> residual tails ------------------------------------------------------------------------------
def affine_code_res(x, scale, shift, code=None, res=None, pre_relu=False, post_relu=False):
    """post_relu?( pre_relu?(x * scale + shift) * code + res ); x [N, ..., C], code [N, C]."""
    x, scale, shift, code, res = _d(x, scale, shift, code, res)
    z = x * scale + shift
    if pre_relu:
        z = z.clamp_min(0.0)
    if code is not None:
        z = z * _per_image(code, x)
    if res is not None:
        z = z + res
    return z.clamp_min(0.0) if post_relu else z


def affine_relu_maxpool2(x, scale, shift):
    """MaxPool2d(2)(relu(x * scale + shift)) on [N, 2 Ho, 2 Wo, C] -> [N, Ho, Wo, C]."""
    x, scale, shift = _d(x, scale, shift)
    z = (x * scale + shift).clamp_min(0.0)
    n, h, w, c = z.shape
    return z.reshape(n, h // 2, 2, w // 2, 2, c).amax(dim=(2, 4))


def code_bn_stats(g, code, x, mean, rstd, scale=None, shift=None, pre_relu=False, y_post=None):
    """First pass of the backward of y = post_relu?( pre_relu?(BN(x)) * code + res ) -> (dz, s1, s2, g_gated):
    g_gated = g [y_post > 0] (g itself without y_post; also the residual's gradient), dz = g_gated code [x scale + shift > 0
    if pre_relu], s1 = sum dz, s2 = sum dz xhat."""
    g, code, x, mean, rstd, scale, shift, y_post = _d(g, code, x, mean, rstd, scale, shift, y_post)
    c = x.shape[-1]
    if y_post is not None:
        g = torch.where(y_post > 0, g, torch.zeros_like(g))
    dz = g if code is None else g * _per_image(code, x)
    if pre_relu:
        dz = torch.where(x * scale + shift > 0, dz, torch.zeros_like(dz))
    xh = (x - mean) * rstd
    return dz, dz.reshape(-1, c).sum(0), (dz * xh).reshape(-1, c).sum(0), g


def code_bn_bwd(g, code, x, scale, mean, rstd, shift=None, pre_relu=False, y_post=None, round_dz=None):
    """Backward of the tail w.r.t. x through the batch statistics -> (dx, dgamma, dbeta, g_gated)."""
    dz, s1, s2, gg = code_bn_stats(g, code, x, mean, rstd, scale, shift, pre_relu, y_post)
    if round_dz is not None:
        dz = round_dz(dz)
    count = dz.numel() // x.shape[-1]
    return bn_apply(dz, x, scale, mean, rstd, s1, s2, count), s2, s1, gg


# ---- losses -----------------------------------------------------------------------------------------------------------
def softplus(a):
    return torch.logaddexp(a.to(F64), torch.zeros((), dtype=F64))


def bce_logits(a, t, gscale=1.0):
    """-> (recon = sigmoid(a), per-element loss t min(softplus(-a), 100) + (1 - t) min(softplus(a), 100), the clamp of
    F.binary_cross_entropy's log terms at -100, and d loss / d a * gscale = (recon - t) gscale)."""
    a, t = _d(a, t)
    r = torch.sigmoid(a)
    loss = t * softplus(-a).clamp_max(100.0) + (1 - t) * softplus(a).clamp_max(100.0)
    return r, loss, (r - t) * gscale


def cross_entropy(logits, target, gscale=1.0):
    """Rows of logits [P, C] -> (logsumexp - logits[target] per row, (softmax - onehot) gscale)."""
    x = logits.to(F64)
    lse = torch.logsumexp(x, -1)
    rows = lse - x.gather(-1, target.view(-1, 1)).view(-1)
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(p).scatter_(-1, target.view(-1, 1), 1.0)
    return rows, (p - onehot) * gscale


def argmin(x):
    """First minimum over the last dimension with torch.argmin's order: NaN ranks below every number (the first NaN wins),
    -0.0 equals 0.0, equal values are ranked by index."""
    x = x.to(F64)
    nan = torch.isnan(x)
    has_nan = nan.any(-1, keepdim=True)
    m = torch.where(nan, torch.full_like(x, float('inf')), x).min(-1, keepdim=True).values
    hit = torch.where(has_nan, nan, x == m)
    ar = torch.arange(x.shape[-1]).expand_as(x)
    return torch.where(hit, ar, torch.full_like(ar, x.shape[-1])).min(-1).values


def mse_tanh(x, t, gscale=1.0):
    """-> (decoded = tanh(x), sum (decoded - t)^2, gscale (decoded - t) (1 - decoded^2))."""
    x, t = _d(x, t)
    r = torch.tanh(x)
    e = r - t
    return r, (e * e).sum(), gscale * e * (1 - r * r)


# ---- VectorQuantization's training step (modules.py:18-43) --------------------------------------------------------------
def vq_step(feat, codes, emb, cs0, mean0, decay, one_m_decay, eps, commit):
    """feat [P, D], codes [P] (the nearest codes), emb [D, K] before the update, cs0 [K] = cluster_size, mean0 [D, K] =
    embedding_mean -> dict: q = E[:, codes]^T, counts, cs / em / e (the three buffers after the EMA update), diff =
    mean (q - f)^2, g = commit * 2 * (f - q) / (P D) (the commitment loss's gradient w.r.t. f)."""
    feat, emb, cs0, mean0 = _d(feat, emb, cs0, mean0)
    p, d = feat.shape
    k = emb.shape[1]
    onehot = torch.nn.functional.one_hot(codes, k).double()
    cnt = onehot.sum(0)
    q = emb[:, codes].t()
    cs = cs0 * decay + one_m_decay * cnt
    em = mean0 * decay + one_m_decay * (feat.t() @ onehot)
    n = cs.sum()
    e = em / ((cs + eps) / (n + k * eps) * n)
    return {'q': q, 'counts': cnt, 'cs': cs, 'em': em, 'e': e, 'diff': ((q - feat) ** 2).mean(),
            'g': commit * 2 * (feat - q) / (p * d), 'onehot': onehot}
