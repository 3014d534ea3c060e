"""Float64 CPU references for the MCGAN kernels of csrc/small_ops.hip: spectral-norm power iteration and gradient fix,
Adam, BatchNorm statistics and backward, column sums; the discriminator tail, the hinge losses, tanh backward, the
MultimodalController codes, compaction maps and affine rows, 2x2 sum pooling and bf16 rounding.  Each function takes the
exact values a kernel read (fp32 scalars passed as their fp32 value, e.g. f32(0.9); bf16 activations as their exact
values) and returns float64 tensors; test_small_ops_ref_cpu.py checks them against torch's own modules,
test_mcgan_small_ops_gpu.py and test_mcgan_tail_code_ops_gpu.py check the kernels against them.  The last section builds
the inputs of test_mcgan_tail_code_ops_gpu.py, so that the CPU test checks that file's input conditions on the same values."""
import math
import zlib

import torch

F64 = torch.float64


def f32(x: float) -> float:
    """The fp32 value a kernel receives for the Python float x."""
    return float(torch.tensor(x, dtype=torch.float32))


def normalize(x):
    """torch.nn.functional.normalize(x, dim=0, eps=1e-12), as the kernels form it: x / max(|x|, eps)."""
    return x / max(float(x.norm()), 1e-12)


def power_v(w, u):
    """First half of a training-mode round (models/utils.py:17-21): v = normalize(W^T u); also returns W^T u."""
    vt = w.to(F64).t() @ u.to(F64)
    return normalize(vt), vt


def power_u(w, v):
    """Second half: t = W v, u = normalize(t), sigma = u . t (= |t|); returns (u, sigma, t)."""
    t = w.to(F64) @ v.to(F64)
    u = normalize(t)
    return u, float(u @ t), t


def power_round(w, u):
    """One training-mode power iteration from u -> (u', v', sigma)."""
    v, _ = power_v(w, u)
    u2, sigma, _ = power_u(w, v)
    return u2, v, sigma


def sigma_eval(w, u, v):
    """Evaluation mode: no iteration, sigma = u . (W v)."""
    return float(u.to(F64) @ (w.to(F64) @ v.to(F64)))


def grad_fix(g, w, u, v, sigma):
    """d(loss)/d(weight_orig) from d(loss)/d(W / sigma) with sigma = u^T W v and u, v held constant (torch's spectral_norm):
    (G - <G, W> / sigma * u v^T) / sigma."""
    g, w, u, v = (x.to(F64) for x in (g, w, u, v))
    d = float((g * w).sum())
    return (g - d / sigma * torch.outer(u, v)) / sigma


def adam(p, g, m, v, t, lr, b1, b2, eps, wd):
    """torch.optim.Adam's update (no amsgrad, weight decay added to the gradient) at step t -> (p', m', v')."""
    p, g, m, v = (x.to(F64) for x in (p, g, m, v))
    if wd != 0:
        g = g + wd * p
    m2 = b1 * m + (1 - b1) * g
    v2 = b2 * v + (1 - b2) * g * g
    bc1 = 1 - b1 ** t
    bc2s = (1 - b2 ** t) ** 0.5
    return p - lr / bc1 * (m2 / (v2.sqrt() / bc2s + eps)), m2, v2


def bn_stats(s1, s2, count, gamma, beta, eps):
    """Training-mode BatchNorm from a channel's sum and sum of squares -> dict of mean, biased var (clamped at 0), rstd,
    scale = gamma rstd, shift = beta - mean scale, unbiased var."""
    s1, s2, gamma, beta = (x.to(F64) for x in (s1, s2, gamma, beta))
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0.0)
    rstd = 1.0 / (var + eps).sqrt()
    scale = gamma * rstd
    unb = var * count / (count - 1) if count > 1 else var
    return {'mean': mean, 'var': var, 'rstd': rstd, 'scale': scale, 'shift': beta - mean * scale, 'unb': unb}


def bn_running(rm, rv, means, unbs, momentum):
    """Running statistics after one update per statistics group, in order (means / unbs: [groups, C])."""
    rm, rv = rm.to(F64), rv.to(F64)
    for mu, ub in zip(means, unbs):
        rm = (1 - momentum) * rm + momentum * mu.to(F64)
        rv = (1 - momentum) * rv + momentum * ub.to(F64)
    return rm, rv


def bn_eval_affine(gamma, beta, rm, rv, eps):
    """Evaluation-mode BatchNorm as an affine map -> (scale, shift)."""
    scale = gamma.to(F64) / (rv.to(F64) + eps).sqrt()
    return scale, beta.to(F64) - rm.to(F64) * scale


def bn_backward(dz, x, count, scale, mean, rstd, s1, s2, add=None):
    """dx of y = scale (x - mean) rstd + shift, channels last, from the batch sums s1 = sum dz, s2 = sum dz xhat:
    scale (dz - s1 / count - xhat s2 / count) (+ add)."""
    dz, x, scale, mean, rstd, s1, s2 = (t.to(F64) for t in (dz, x, scale, mean, rstd, s1, s2))
    xh = (x - mean) * rstd
    dx = scale * (dz - s1 / count - xh * s2 / count)
    return dx if add is None else dx + add.to(F64)


def colsum(x, c, alpha=1.0, row_perm=1):
    """alpha * sum over the leading dims of x[..., :c]; row_perm > 1 stores column j = k Cc + i at i row_perm + k."""
    s = alpha * x.to(F64).reshape(-1, x.shape[-1])[:, :c].sum(0)
    if row_perm > 1:
        s = s.view(row_perm, c // row_perm).t().reshape(-1)
    return s


# ---- the tail, hinge, code and layout kernels (test_mcgan_tail_code_ops_gpu.py) -------------------------------------------
def round_bf16(x):
    """Round-to-nearest-even of fp32 values (given as float64) to bf16 -> float64.  Integer arithmetic on the fp32 bit
    pattern: add 0x7FFF plus the lowest kept bit, drop the low 16 bits."""
    x32 = x.to(torch.float32)
    assert bool((x32.to(F64) == x.to(F64)).all()), 'round_bf16 takes fp32 values'
    bits = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    r = torch.where(r >= 2 ** 31, r - 2 ** 32, r).to(torch.int32)
    return r.view(torch.float32).to(F64).reshape(x.shape)


def quantum(*ts):
    """The largest power of two <= 1 that divides every entry of the tensors."""
    k = 0
    for t in ts:
        t = torch.as_tensor(t, dtype=F64).reshape(-1)
        while k < 60 and not bool((t * 2.0 ** k == torch.round(t * 2.0 ** k)).all()):
            k += 1
    return 2.0 ** -k


def sum_bits(mag, q):
    """Significand bits an integer multiple of q of magnitude <= mag can need."""
    return 0 if mag <= 0 else int(math.floor(math.log2(mag / q))) + 1


def assert_exact(bits, what=''):
    """The condition on the INPUTS under which fp32 sums are exact in any order: every partial sum is a multiple of the
    terms' quantum and bounded by the sum of their magnitudes, so it fits fp32's 24-bit significand."""
    assert bits <= 24, f'{what}: a partial sum can need {bits} bits: the inputs are too large for exact fp32 sums'


def dtail(x, code, w, b, sigma):
    """Discriminator tail (mcgan.py:158-165): x [N, HW, C], code [N, C] or None, w [C], b and sigma numbers ->
    dict(pooled [N, C] = code * sum_hw relu(x), logit [N] = pooled . w / sigma + b,
         pooled_abs [N, C] = sum |term| of a pooled entry (|code| sum_hw relu(x)),
         logit_abs [N] = sum_c |pooled_c w_c / sigma| + |b|, wn = w / sigma)."""
    x, w = x.to(F64), w.to(F64)
    s = x.clamp_min(0.0).sum(1)
    cd = torch.ones_like(s) if code is None else code.to(F64)
    pooled = s * cd
    wn = w / float(sigma)
    logit = (pooled * wn).sum(1) + float(b)
    return {'pooled': pooled, 'logit': logit, 'pooled_abs': s * cd.abs(),
            'logit_abs': (pooled * wn).abs().sum(1) + abs(float(b)), 'wn': wn}


def dtail_dx(dlogit, x, code, w, sigma):
    """d logit / d x times dlogit: dlogit[n] w[c] / sigma code[n, c] where x > 0, else 0 -> (dx [N, HW, C], mask x > 0)."""
    x = x.to(F64)
    g = dlogit.to(F64).view(-1, 1) * (w.to(F64) / float(sigma)).view(1, -1)
    if code is not None:
        g = g * code.to(F64)
    mask = x > 0
    return g.unsqueeze(1) * mask, mask


def dtail_wgrad(dlogit, pooled):
    """Tail weight / bias gradients wrt the normalised weight: dw[c] = sum_n dlogit[n] pooled[n, c], db = sum_n dlogit[n]
    -> (dw, db, dw_abs, db_abs), the last two the sums of the terms' magnitudes."""
    t = dlogit.to(F64).view(-1, 1) * pooled.to(F64)
    return t.sum(0), dlogit.to(F64).sum(), t.abs().sum(0), dlogit.to(F64).abs().sum()


def dtail_pair_wgrad(dlogit, pooled, ratio):
    """The paired form: rows [0, N) -> (dw1, db1), rows [N, 2N) -> (dw2 / ratio, db2); each as dtail_wgrad returns it."""
    n = dlogit.numel() // 2
    first = dtail_wgrad(dlogit[:n], pooled[:n])
    dw, db, dwa, dba = dtail_wgrad(dlogit[n:], pooled[n:])
    return first, (dw / float(ratio), db, dwa / abs(float(ratio)), dba)


def hinge_d(real, fake):
    """train_gan.py:154: loss = mean relu(1 - real) + mean relu(1 + fake) -> (loss, dreal, dfake, loss_abs); the gradient
    of relu at 0 is 0, as torch's."""
    real, fake = real.to(F64), fake.to(F64)
    n = real.numel()
    r, f = 1.0 - real, 1.0 + fake
    loss = r.clamp_min(0).sum() / n + f.clamp_min(0).sum() / n
    return loss, -(r > 0).to(F64) / n, (f > 0).to(F64) / n, loss


def hinge_g(fake):
    """train_gan.py:172: loss = -mean(fake) -> (loss, dfake, loss_abs)."""
    fake = fake.to(F64)
    n = fake.numel()
    return -fake.sum() / n, torch.full_like(fake, -1.0 / n), fake.abs().sum() / n


def tanh_bwd(dy, y):
    """nn.Tanh backward from its output: dy (1 - y^2)."""
    return dy.to(F64) * (1.0 - y.to(F64) ** 2)


def mc_code(indicator, codebook, n_half=None, scale=None):
    """MultimodalController.forward's code (modules.py:73): indicator @ codebook; rows n >= n_half times scale."""
    code = indicator.to(F64) @ codebook.to(F64)
    if scale is not None:
        code = code.clone()
        code[n_half:] *= float(scale)
    return code


def cmap_record(code_row):
    """One record of mcgen_mc_cmap as include/mcgen_hip.h documents it -> (cpos [C], cidx [C + 32], cpre [ceil(C / 32) + 1])
    as int64: the position of every channel among the active ones (code != 0; -0.0 is inactive, a negative entry active) or
    -1, the active channels in order padded with C, the number of active channels below every 32-channel boundary."""
    c = code_row.numel()
    active = (code_row.to(F64) != 0).nonzero().flatten()
    cpos = torch.full((c,), -1, dtype=torch.int64)
    cpos[active] = torch.arange(active.numel())
    cidx = torch.full((c + 32,), c, dtype=torch.int64)
    cidx[:active.numel()] = active
    nd = (c + 31) // 32
    cpre = torch.tensor([int((active < 32 * d).sum()) for d in range(nd)] + [active.numel()], dtype=torch.int64)
    return cpos, cidx, cpre


def mc_affine_rows(code, ccap, scale=None, shift=None, group_n=0):
    """mcgen_mc_affine: slot j of image n holds (scale[n // group_n][c] or 1) * code[n][c] and (shift[...][c] or 0) *
    code[n][c] for c = the image's j-th active channel; slots past the active count hold 0 -> (scale_out, shift_out)."""
    n, c = code.shape
    code = code.to(F64)
    so, ho = torch.zeros(n, ccap, dtype=F64), torch.zeros(n, ccap, dtype=F64)
    for i in range(n):
        act = cmap_record(code[i])[1][:ccap]
        act = act[act < c]
        g = i // group_n if group_n > 0 else 0
        cd = code[i, act]
        so[i, :act.numel()] = cd if scale is None else scale.to(F64).view(-1, c)[g, act] * cd
        if shift is not None:
            ho[i, :act.numel()] = shift.to(F64).view(-1, c)[g, act] * cd
    return so, ho


def pool2_sum(x):
    """2x2 sums of x [N, 2 Ho, 2 Wo, C] -> (sums, sums of magnitudes)."""
    x = x.to(F64)
    p = lambda t: t[:, 0::2, 0::2] + t[:, 0::2, 1::2] + t[:, 1::2, 0::2] + t[:, 1::2, 1::2]
    return p(x), p(x.abs())


# ---- inputs that the CPU test and the GPU test both build, so the input conditions are checked on the same values ----------
U32 = 2.0 ** -24
TAIL_SHAPES = [(3, 8, 16), (5, 24, 9), (4, 128, 64), (4, 200, 16), (3, 512, 16), (2, 1024, 7), (2, 1032, 4), (2, 2048, 4)]
TAIL_SCALAR_SHAPES = [(3, 12, 16), (1, 2056, 2)]
TAIL_EXACT_SHAPES = [(8, 8, 16), (8, 24, 9), (8, 128, 64), (8, 512, 16), (8, 1032, 4), (8, 2048, 4)]
FUSED_RANDOM = [(n + n % 2, c, hw) for n, c, hw in TAIL_SHAPES] + [(2, 40, 5)]        # d_pair needs an even N; N = 2: one real, one generated


# random fused-tail cases (N, C, HW, bf16, with_code) whose first seed puts a reference logit within four bounds of a hinge
# point: they take another seed (test_random_fused_tail_cases_have_no_undecided_sample holds for the table as it stands)
FUSED_SALT = {(2, 1024, 7, True, False): (1,)}


def fused_inputs(n, c, hw, bf16, with_code):
    return tail_inputs(n, c, hw, bf16, with_code, *FUSED_SALT.get((n, c, hw, bf16, with_code), ()))


def seed_of(*key):
    return zlib.crc32(repr(key).encode()) % 100003


def tail_inputs(n, c, hw, bf16, with_code, *salt):
    """Random tail inputs: x [N, HW, C] (bf16 values when `bf16`) with about 1 in 16 entries 0.0 and 1 in 16 -0.0, a
    non-negative code with about half its entries zero (or None), w, b, sigma as fp32 values -> dict of fp32 tensors."""
    gen = torch.Generator().manual_seed(seed_of('tail', n, c, hw, bf16, with_code, *salt))
    x = torch.randn(n, hw, c, generator=gen)
    pick = torch.randint(0, 16, (n, hw, c), generator=gen)
    x[pick == 0] = 0.0
    x[pick == 1] = -0.0
    x[:, 0::2, c - 1] = 0.0                  # the last channel holds nothing but zeros of both signs: it pools as exactly 0
    x[:, 1::2, c - 1] = -0.0
    if bf16:
        x = x.bfloat16().float()
    code = None
    if with_code:
        code = (torch.rand(n, c, generator=gen) < 0.5).float() * (0.5 + torch.rand(n, c, generator=gen))
    w = torch.randn(c, generator=gen) * (4.0 / c ** 0.5)
    b = torch.randn(1, generator=gen)
    return {'x': x, 'code': code, 'w': w, 'b': b, 'sigma': torch.tensor([1.7])}


def tail_bounds(t, ref):
    """-> (tol_pooled [N, C], tol_logit [N]) from the reference alone: pooled is a chain of HW - 1 additions and one
    product, HW u sum |terms|; logit carries that through |w / sigma| and adds C fmas, the bias and the division of
    w by sigma, (C + 2) u sum |terms|, doubled for a division within 2u and the second-order terms."""
    n, hw, c = t['x'].shape
    tol_p = hw * U32 * ref['pooled_abs']
    tol_l = (tol_p * ref['wn'].abs()).sum(1) + 2 * (c + 2) * U32 * ref['logit_abs']
    return tol_p, tol_l


def undecided(ref, tol_logit, mode):
    """Samples whose reference logit lies within 4 tol of the hinge point that decides their gradient (d_pair: +1 for the
    first half, -1 for the second; g: none)."""
    if mode == 'g':
        return torch.zeros_like(ref['logit'], dtype=torch.bool)
    n = ref['logit'].numel()
    point = torch.cat([torch.ones(n // 2, dtype=F64), -torch.ones(n - n // 2, dtype=F64)])
    return (ref['logit'] - point).abs() <= 4 * tol_logit


def tail_exact_inputs(n, c, hw, with_code=True):
    """Dyadic tail inputs on which every fp32 partial sum is exact in any order: x integers in [-3, 3] (some -0.0), code
    in {0, 1}, w multiples of 2^-4 in [-1, 1], sigma = 2, and b such that, with h = N / 2, samples 0 and h have logit
    exactly +1, samples 1 and h + 1 exactly -1, samples 2 and h + 2 exactly 0.  Channel 0 has w = 2 (w / sigma = 1) and
    code 1; x[:, 1:, 0] <= 0, so x[n, 0, 0] in {2, 0, 1} adds exactly that to the logit of the copies of sample 0."""
    assert n >= 8 and n % 2 == 0
    gen = torch.Generator().manual_seed(seed_of('tail exact', n, c, hw, with_code))
    x = torch.randint(-3, 4, (n, hw, c), generator=gen).float()
    x[(x == 0) & (torch.rand(n, hw, c, generator=gen) < 0.5)] = -0.0
    code = (torch.rand(n, c, generator=gen) < 0.5).float() if with_code else None
    w = torch.randint(-16, 17, (c,), generator=gen).float() / 16
    w[0] = 2.0
    x[:, 1:, 0] = -x[:, 1:, 0].abs()
    if code is not None:
        code[:, 0] = 1.0
    h = n // 2
    for base in (0, h):
        for k, v in enumerate((2.0, 0.0, 1.0)):
            x[base + k] = x[0]
            x[base + k, 0, 0] = v
            if code is not None:
                code[base + k] = code[0]
    sigma = torch.tensor([2.0])
    b0 = dtail(x[:1], None if code is None else code[:1], w, 0.0, 2.0)['logit'][0]
    b = torch.tensor([1.0 - float(b0)])
    return {'x': x, 'code': code, 'w': w, 'b': b, 'sigma': sigma}


def tail_exact_bits(t):
    """The bits any partial sum of the exact tail case can need: pooled (integers up to 3 HW), the logit (multiples of the
    quantum of w / sigma and b, bounded by sum |terms| + |b|), from the reference alone."""
    ref = dtail(t['x'], t['code'], t['w'], t['b'], t['sigma'])
    q = min(quantum(ref['wn']) * quantum(ref['pooled']), quantum(t['b']))
    return max(sum_bits(float(ref['pooled_abs'].max()), quantum(t['x'])), sum_bits(float(ref['logit_abs'].max()), q))


def pool_exact_input(n, h, w, c, seed):
    """Multiples of 1/4 in [-4, 4]: bf16 values whose 2x2 sums are bf16 values too (6 bits at most)."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-16, 17, (n, h, w, c), generator=gen).float() / 4
