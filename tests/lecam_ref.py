"""Float64 CPU references for the LeCam regulariser of the discriminator loss (Tseng et al., "Regularizing GANs under
Limited Data", CVPR 2021; include/mcgen_hip.h: mcgen_lecam_state_t), the error bounds the GPU tests hold the three kernel
entries to (mcgen_lecam_loss_d, mcgen_dtail_lecam_fused, mcgen_dtail_pair_wgrad_lecam_loss), and the CPU oracle with the
regulariser in its D-loss line.  This file is the specification; test_lecam_ref_cpu.py checks it against torch's own
float64 autograd of the written-out loss.

Definition.  State: anchors a_R, a_F (fp32, initially 0) and the count t of discriminator updates done (initially 0).
For update t with N real logits r_i and N generated logits f_i, anchors as they stand BEFORE the update:
    active = lambda > 0 and t >= start
    R      = mean (r_i - a_F)^2 + mean (f_i - a_R)^2
    loss   = base(loss_type) + (lambda R if active else 0)
    d/dr_i = base_i + (2 lambda (r_i - a_F) / N if active else 0)          (f_i likewise, with a_R)
the anchors being constants of the differentiation.  Then m_R = mean r_i, m_F = mean f_i, r_t = mean sign(r_i) with
sign(0) = 0, and a = m if t == 0 else decay a + (1 - decay) m for both anchors, and t += 1 -- before `start` as well.

Bounds (u = 2^-24; gan_loss_ref's assumptions; the inputs -- logits, anchors, lambda and decay -- are fp32 numbers, which
the references take exactly, so only the kernel's own operations are bounded; "doubled" = the allowance gan_loss_ref
makes for second-order terms):
- the term T = 2 lambda (l - a) / N is formed as fl(fl((2 lambda) fl(l - a)) fl(1 / N)): the subtraction's error is
  u |l - a|, which the two products and the rounding of 1 / N carry on and add one u each to: 4u |T| in all.  (2 lambda
  is exact: a power-of-two scaling.)
- d = fl(base + T): the base derivative's own bound -- hinge: the rounding of 1 / N, u |base| (the decision 1 -+ l > 0 is
  exact: fl(1 -+ l) has the sign of 1 -+ l); BCE: gan_loss_ref.grad_tol -- plus the term's 4u |T| plus the addition's
  u |base + T| <= u (|base| + |T|); term and addition doubled: base_tol + 2 (5u |T| + u |base|) + TINY.
- the sum of squares Q = sum (l - a)^2: each term carries the subtraction twice and one product, 3u; N - 1 additions in
  any order, the rounding of 1 / N and the product by it, (N + 2) u; doubled: 2 (3 + N + 2) u Q / N per half.  R is the
  sum of the two halves: one more u R, doubled.
- loss = fl(base + fl(lambda R)): the base loss's bound -- BCE: gan_loss_ref.loss_tol; hinge: the same formula with one
  rounding per term (the subtraction 1 -+ l), 2 (u + (N + 2) u) sum terms / N -- plus lambda times R's bound plus the
  product and the addition, u lambda R + u |loss|, doubled.
- m = fl(sum l fl(1 / N)): 2 (N + 2) u mean |l|.  r_t: the sum of N <= 2^24 values of -1, 0, 1 is exact; 1 / N and the
  product: 2 * 2u |r_t|.
- the moved anchor a' = fl(fl(decay a) + fl(fl(1 - decay) m)) (t > 0): m's bound times (1 - decay), then
  u |decay a| + 2u |(1 - decay) m| + u |a'|, doubled; t == 0: a' = m, m's bound.
"""
import torch
import torch.nn.functional as F

import gan_loss_ref as G
from oracle import mcgan_oracle as O

F64 = torch.float64
U32 = G.U32
TINY = G.TINY
LOSS_IDS = {'Hinge': 0, 'BCE': 1}


def f32(v):
    """A Python number as the fp32 value a kernel argument holds, in float64."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def fresh_state():
    return {'a_R': 0.0, 'a_F': 0.0, 't': 0}


def base_d(real, fake, loss_type):
    """-> (loss, dreal, dfake, terms): the discriminator loss without the regulariser, float64; `terms`: the 2N
    non-negative summands, not yet divided by N."""
    real, fake = real.to(F64), fake.to(F64)
    n = real.numel()
    if loss_type == 'BCE':
        loss, dr, df, _ = G.bce_d(real, fake)
        return loss, dr, df, torch.cat([G.softplus(-real), G.softplus(fake)])
    if loss_type != 'Hinge':
        raise ValueError('Not valid loss type')
    tr, tf = (1.0 - real).clamp_min(0.0), (1.0 + fake).clamp_min(0.0)
    dr = (1.0 - real > 0).to(F64) * (-1.0 / n)
    df = (1.0 + fake > 0).to(F64) * (1.0 / n)
    return tr.sum() / n + tf.sum() / n, dr, df, torch.cat([tr, tf])


def base_grad_tol(d, loss_type):
    return G.grad_tol(d) if loss_type == 'BCE' else U32 * d.to(F64).abs()


def base_loss_tol(terms, n, loss_type):
    if loss_type == 'BCE':
        return G.loss_tol(terms, n)
    terms = terms.to(F64)
    return 2 * (U32 * terms.sum() + (n + 2) * U32 * terms.sum()) / n


def lecam_d(real, fake, loss_type, state, lam, decay, start):
    """One discriminator loss with the regulariser, float64, from the fp32 logits `real` / `fake` [N] and
    state = {'a_R', 'a_F', 't'} -> a dict:
      loss, dreal, dfake                       the values of the definition
      loss_tol, dreal_tol, dfake_tol           the module docstring's bounds
      active, R, R_tol, stats = {'m_R', 'm_F', 'r_t'}, stats_tol (same keys)
      state = {'a_R', 'a_F', 't'} after the update, anchor_tol = {'a_R', 'a_F'}
    The fused tail's dlogit of a paired batch is cat(dreal, dfake); the paired tail-gradient launch owes loss, stats and state."""
    real, fake = real.detach().cpu().to(F64).reshape(-1), fake.detach().cpu().to(F64).reshape(-1)
    n = real.numel()
    assert fake.numel() == n and n > 0
    lam, decay = f32(lam), f32(decay)
    a_r, a_f, t = f32(state['a_R']), f32(state['a_F']), int(state['t'])
    active = lam > 0 and t >= int(start)
    loss, dr, df, terms = base_d(real, fake, loss_type)
    out = {'active': active}
    sq_r, sq_f = (real - a_f) ** 2, (fake - a_r) ** 2
    reg = sq_r.sum() / n + sq_f.sum() / n
    half_tol = lambda q: 2 * (3 + n + 2) * U32 * q.sum() / n
    reg_tol = half_tol(sq_r) + half_tol(sq_f) + 2 * U32 * reg + TINY
    out['R'], out['R_tol'] = reg, reg_tol
    ltol = base_loss_tol(terms, n, loss_type)
    gr_tol, gf_tol = base_grad_tol(dr, loss_type), base_grad_tol(df, loss_type)
    if active:
        t_r, t_f = 2 * lam * (real - a_f) / n, 2 * lam * (fake - a_r) / n
        gr_tol = gr_tol + 2 * (5 * U32 * t_r.abs() + U32 * dr.abs()) + TINY
        gf_tol = gf_tol + 2 * (5 * U32 * t_f.abs() + U32 * df.abs()) + TINY
        dr, df = dr + t_r, df + t_f
        ltol = ltol + lam * reg_tol + 2 * (U32 * lam * reg + U32 * (loss + lam * reg).abs())
        loss = loss + lam * reg
    out.update(loss=loss, dreal=dr, dfake=df, loss_tol=ltol + TINY, dreal_tol=gr_tol, dfake_tol=gf_tol)
    m_r, m_f = real.sum() / n, fake.sum() / n
    m_tol = lambda l: 2 * (n + 2) * U32 * l.abs().sum() / n + TINY
    r_t = torch.sign(real).sum() / n
    out['stats'] = {'m_R': m_r, 'm_F': m_f, 'r_t': r_t}
    out['stats_tol'] = {'m_R': m_tol(real), 'm_F': m_tol(fake), 'r_t': 4 * U32 * r_t.abs()}

    def move(a, m, mt):
        if t == 0:
            return m, mt
        new = decay * a + (1 - decay) * m
        return new, (1 - decay) * mt + 2 * (U32 * abs(decay * a) + 2 * U32 * ((1 - decay) * m).abs() + U32 * new.abs()) + TINY
    new_r, tol_r = move(a_r, m_r, out['stats_tol']['m_R'])
    new_f, tol_f = move(a_f, m_f, out['stats_tol']['m_F'])
    out['state'] = {'a_R': float(new_r), 'a_F': float(new_f), 't': t + 1}
    out['anchor_tol'] = {'a_R': float(tol_r), 'a_F': float(tol_f)}
    return out


def written_out_loss(real, fake, loss_type, state, lam, start):
    """The loss as one differentiable float64 expression of `real` / `fake` (autograd tensors): what lecam_d's gradients
    are checked against."""
    n = real.numel()
    if loss_type == 'BCE':
        loss = F.binary_cross_entropy_with_logits(real, torch.ones_like(real)) + \
            F.binary_cross_entropy_with_logits(fake, torch.zeros_like(fake))
    else:
        loss = torch.relu(1.0 - real).mean() + torch.relu(1.0 + fake).mean()
    if f32(lam) > 0 and int(state['t']) >= int(start):
        loss = loss + f32(lam) * (((real - f32(state['a_F'])) ** 2).sum() / n + ((fake - f32(state['a_R'])) ** 2).sum() / n)
    return loss


class OracleMCGANLeCam(O.OracleMCGAN):
    """oracle.mcgan_oracle.OracleMCGAN with the regulariser: `train_iteration` is the oracle's own with its D-loss line
    extended by lambda R and the anchors moved after every discriminator update, as the definition says (fp32 tensors,
    as the oracle computes).  `loss_type` 'BCE' takes gan_loss_ref.OracleMCGANBCE's loss lines.  self.lecam: the state."""

    def __init__(self, state, classes, lam, decay=0.99, start=0, loss_type='Hinge', lecam=None, **k):
        super().__init__(state, classes, **k)
        self.lam, self.decay, self.start, self.loss_type = float(lam), float(decay), int(start), loss_type
        self.lecam = dict(lecam) if lecam is not None else fresh_state()
        self.stats = {}

    def d_loss(self, d_x, d_gz):
        n = d_x.size(0)
        if self.loss_type == 'BCE':
            loss = F.binary_cross_entropy_with_logits(d_x, torch.ones((n, 1))) + \
                F.binary_cross_entropy_with_logits(d_gz, torch.zeros((n, 1)))
        else:
            loss = torch.relu(1.0 - d_x).mean() + torch.relu(1.0 + d_gz).mean()
        s = self.lecam
        if self.lam > 0 and s['t'] >= self.start:
            loss = loss + self.lam * (((d_x - s['a_F']) ** 2).mean() + ((d_gz - s['a_R']) ** 2).mean())
        with torch.no_grad():
            m_r, m_f = float(d_x.mean()), float(d_gz.mean())
            self.stats = {'m_R': m_r, 'm_F': m_f, 'r_t': float(torch.sign(d_x).mean())}
            if s['t'] == 0:
                s['a_R'], s['a_F'] = m_r, m_f
            else:
                s['a_R'] = self.decay * s['a_R'] + (1 - self.decay) * m_r
                s['a_F'] = self.decay * s['a_F'] + (1 - self.decay) * m_f
            s['t'] += 1
        return loss

    def train_iteration(self, img, label, zs):
        zi = iter(zs)
        n = img.size(0)
        for _ in range(self.d_iters):
            self._zero()
            d_x = self.discriminate(img, label)
            fake = self.generate(label, next(zi))
            d_gz = self.discriminate(fake.detach(), label)
            d_loss = self.d_loss(d_x, d_gz)
            d_loss.backward()
            self.opt_d.step()
        for _ in range(self.g_iters):
            self._zero()
            fake = self.generate(label, next(zi))
            d_gz = self.discriminate(fake, label)
            g_loss = F.binary_cross_entropy_with_logits(d_gz, torch.ones((n, 1))) if self.loss_type == 'BCE' else -d_gz.mean()
            g_loss.backward()
            self.opt_g.step()
        return float(d_loss.detach()), float(g_loss.detach())
