"""float64 reference of the incremental PixelCNN sampler (csrc/pixelcnn_sample.hip), for test_px_sample_ref_cpu.py and
test_px_sample_kernels_gpu.py: a plain whole-map eval forward of MCGatedPixelCNN / ConditionalGatedPixelCNN from a state
dict, the inverse-CDF draw, and the logit vectors and `u` probes the draw is tested at.

`forward64` is a second statement of the operation, independent of the row / column schedule that
test_pixelcnn_sample_cpu.schedule_forward restates: every layer is a masked F.conv2d over the whole map, cropped per
coordinate (rows to H, columns to W), so a non-square map is causal."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5                      # BatchNorm eps of every layer
MARGIN = 1e-5                   # distance of every interval probe from the nearest CDF boundary, as a fraction of S
P_MIN = 4e-5                    # a code is probed when its probability is at least this (room for two margins and more)
FP32_TINY = 2.0 ** -149         # the smallest fp32 denormal: a mass below it is 0 in fp32, flushed or not


# ---- models ---------------------------------------------------------------------------------------------------------------
def build(name, hidden, layers, codes, modes=10, device='cpu', seed=1):
    """models.mcpixelcnn() / models.cpixelcnn() at the given widths in eval mode, every float parameter and running
    statistic randomised as test_pixelcnn_sample_cpu.test_row_column_schedule_matches_oracle does, mask A applied."""
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    saved = dict(cfg)
    try:
        cfg.update(model_name=name, device=device, classes_size=modes, controller_rate=0.5, compute_dtype='float32')
        cfg['pixelcnn'] = {'num_layer': layers, 'hidden_size': hidden, 'num_embedding': codes}
        torch.manual_seed(0)
        m = getattr(models, name)()
    finally:
        cfg.clear()
        cfg.update(saved)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for key, t in m.state_dict().items():
            if t.is_floating_point() and 'codebook' not in key:
                t.copy_(torch.randn(t.shape, generator=g) * 0.3)
            if 'running_var' in key:
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    m.layers[0].make_causal()
    return m.to(device).train(False)


def state(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


# ---- the forward ----------------------------------------------------------------------------------------------------------
def forward64(sd, codes, label, classes, conditional, store=None):
    """Eval-mode logits [N, K, H, W] in float64 of the code map `codes` [N, H, W] under `label` [N].  store=torch.bfloat16
    rounds the embedding, every weight, and the activations the kernels store in the compute dtype (pre-gate h_vert, out_v,
    s, out_h, the residual conv, x_h, the head conv, z, the logits); vert_to_horiz stays unrounded."""
    rd = (lambda t: t.to(store).double()) if store is not None else (lambda t: t)
    d = {k: v.detach().double().cpu() for k, v in sd.items() if v.is_floating_point()}
    wrap = '' if conditional else 'module.'
    last = 'output_conv.3.' if conditional else 'output_conv.4.module.'
    n_layer = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('layers.'))
    codes, label = codes.cpu(), label.cpu()
    n, h, w = codes.shape
    onehot = F.one_hot(label, classes).double()

    def affine(x, p):
        sc = d[p + 'weight'] / torch.sqrt(d[p + 'running_var'] + EPS)
        return x * sc[None, :, None, None] + (d[p + 'bias'] - d[p + 'running_mean'] * sc)[None, :, None, None]

    def code(key):                                   # a MultimodalController's row per sample; 1 in the conditional form
        return 1.0 if conditional else (onehot @ d[key])[:, :, None, None]

    def gate(x, p, l, mc_key):
        if conditional:
            x = x + d[f'layers.{l}.class_cond_embedding.weight'][label][:, :, None, None]
        a, b = x.chunk(2, dim=1)
        return code(mc_key) * torch.relu(affine(a, p + 'bn.')) * torch.sigmoid(b)

    x_v = x_h = rd(d['embedding.weight'])[codes].permute(0, 3, 1, 2)
    for l in range(n_layer):
        p = f'layers.{l}.'
        k2 = 3 if l == 0 else 1
        wv, wh = d[p + 'vert_stack.weight'].clone(), d[p + 'horiz_stack.weight'].clone()
        if l == 0:                                   # mask A: neither the current row nor the current column
            wv[:, :, -1] = 0
            wh[:, :, :, -1] = 0
        h_vert = rd(F.conv2d(x_v, rd(wv), d[p + 'vert_stack.bias'], padding=(k2, k2))[:, :, :h, :])
        v2h = F.conv2d(h_vert, rd(d[p + 'vert_to_horiz.weight']), d[p + 'vert_to_horiz.bias'])
        out_v = rd(gate(h_vert, p + 'gate_v.', l, p + 'gate_v.mc.codebook'))
        s = rd(F.conv2d(x_h, rd(wh), d[p + 'horiz_stack.bias'], padding=(0, k2))[:, :, :, :w] + v2h)
        out_h = rd(gate(s, p + 'gate_h.', l, p + 'gate_h.mc.codebook'))
        r = rd(F.conv2d(out_h, rd(d[p + f'horiz_resid.0.{wrap}weight']), d[p + f'horiz_resid.0.{wrap}bias']))
        r = affine(r, p + f'horiz_resid.1.{wrap}') * code(p + 'horiz_resid.2.codebook')
        x_h = rd(r + x_h) if l > 0 else rd(r)
        x_v = out_v
    h0 = rd(F.conv2d(x_h, rd(d[f'output_conv.0.{wrap}weight']), d[f'output_conv.0.{wrap}bias']))
    z = rd(torch.relu(affine(h0, f'output_conv.1.{wrap}')) * code('output_conv.3.codebook'))
    return rd(F.conv2d(z, rd(d[last + 'weight']), d[last + 'bias']))


# ---- the draw -------------------------------------------------------------------------------------------------------------
def _cdf(logits):
    x = logits.double()
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    e = torch.where(e < FP32_TINY, torch.zeros_like(e), e)
    return e, e.cumsum(-1)


def inverse_cdf64(logits, u):
    """logits [R, K] (or [K], shared by every row), u [R] -> (code [R], distance [R] of u * S from the nearest CDF boundary
    as a fraction of S).  Masses are exp(x - max) in float64, 0 below 2^-149; the code is the smallest k with cs_k > u * S,
    and for u * S >= S the last code with mass."""
    u = u.double().reshape(-1)
    if logits.dim() == 1:
        logits = logits[None].expand(u.numel(), -1)
    e, cs = _cdf(logits)
    s = cs[:, -1:]
    t = u[:, None] * s
    k = (cs <= t).sum(-1)
    kq = logits.shape[-1]
    last = (kq - 1) - (e.flip(-1) > 0).double().argmax(-1)
    k = torch.where(t[:, 0] >= s[:, 0], last, k)
    bounds = torch.cat([torch.zeros_like(s), cs], -1)
    return k, ((bounds - t).abs().min(-1).values / s[:, 0])


# ---- draw cases: logit vectors exactly representable in bf16 --------------------------------------------------------------
def _flat(kq):
    return torch.zeros(kq)


def _gauss(kq):
    x = torch.randn(kq, generator=torch.Generator().manual_seed(kq)) * 2
    return ((x * 8).round() / 8).clamp(-8, 8)


def shifted_peaks(kq):
    return [kq * (2 * i + 1) // 10 for i in range(5)]


def _shifted(kq):
    """exp(100) overflows fp32 unless the maximum is subtracted; the gap of 80 leaves every mass normal in fp32."""
    x = torch.full((kq,), 20.0)
    x[shifted_peaks(kq)] = 100.0
    return x


def _sparse(kq):
    """exp(-150) is exactly 0 in fp32: no mass before, between and after the two live codes."""
    x = torch.full((kq,), -150.0)
    x[[3, kq - 5]] = 0.0
    return x


DRAW_CASES = [('flat', kq) for kq in (10, 64, 65, 100, 512)] + [('gauss', 100), ('gauss', 512)] + \
             [('shifted', 100), ('shifted', 512)] + [('sparse', 65), ('sparse', 512)]
_MAKERS = {'flat': _flat, 'gauss': _gauss, 'shifted': _shifted, 'sparse': _sparse}
EDGE_U = (0.0, 1.0 - 2.0 ** -24, 1.0)


def case_logits(name, kq):
    x = _MAKERS[name](kq).float()
    assert torch.equal(x.bfloat16().float(), x), 'a draw case must be exact in bf16'
    return x


def _f32_above(v):
    """The second fp32 at or above v: one ulp of slack, so that the float64 distance from v's side never rounds short."""
    f = torch.tensor(v, dtype=torch.float32)
    f = f if float(f) >= v else torch.nextafter(f, torch.tensor(math.inf))
    return torch.nextafter(f, torch.tensor(math.inf))


def _f32_below(v):
    f = torch.tensor(v, dtype=torch.float32)
    f = f if float(f) <= v else torch.nextafter(f, torch.tensor(-math.inf))
    return torch.nextafter(f, torch.tensor(-math.inf))


def probes(logits):
    """-> (u fp32 [P], probed codes): for every code with p_k >= P_MIN the midpoint of its CDF interval and the points MARGIN
    inside either end (rounded to fp32 towards the inside), then u = 0, 1 - 2^-24 and 1.  Derived from the reference alone."""
    _, cs = _cdf(logits[None])
    cs = cs[0]
    s = float(cs[-1])
    us, probed = [], []
    for k in range(logits.numel()):
        lo, hi = (float(cs[k - 1]) if k else 0.0) / s, float(cs[k]) / s
        if hi - lo < P_MIN:
            continue
        probed.append(k)
        us += [torch.tensor((lo + hi) / 2, dtype=torch.float32), _f32_above(lo + MARGIN), _f32_below(hi - MARGIN)]
    us += [torch.tensor(v, dtype=torch.float32) for v in EDGE_U]
    return torch.stack(us), probed
