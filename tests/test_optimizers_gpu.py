"""SGD, RMSprop and Adamax on the HIP path (csrc/optim_ops.hip; trainer.FusedSGD / FusedRMSprop / FusedAdamax): the
kernels against the float64 restatements of tests/optim_ref.py (pinned to torch.optim in test_optimizers_cpu.py), the
trainers' steps against the same restatements on the trainers' own gradients, graph replay, and resume.

Bounds: u = 2^-24 is the fp32 unit roundoff; a correctly rounded fp32 operation (fma, product, sum, sqrt) has relative
error <= u, a division is taken as within 1 ulp (<= 2u).  Each _*_tol counts the roundings of every term of the kernel's
arithmetic, scales them by the term's magnitude and carries the state's error into p; the result is doubled, which covers
second-order terms.  The references use exactly the fp32 values of the hyper-parameters the kernel receives (R.f32)."""
import pytest
import torch

import golden_util as gu
import optim_ref as OR
import small_ops_ref as R

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
NAN = float('nan')
# thresholds that live only in csrc/optim_ops.hip
OPT_BLOCK = 256         # threads per block
OPT_GRID_CAP = 256      # blocks at most
VEC = 4                 # floats per f32x4 access: the vector loops cover n // 4 vectors, a scalar loop the last n % 4 elements
ONE_TRIP = VEC * OPT_GRID_CAP * OPT_BLOCK    # up to here a lane moves one vector; above, the grid is capped and the two-vector loop runs
# 1, 3: scalar loop only; 4: one vector; 5: a vector and a scalar; ONE_TRIP + 3: the largest n without the two-vector loop
# (tail of 3); ONE_TRIP + 4: lane 0 takes a two-vector trip; 2 * ONE_TRIP: every lane one two-vector trip and nothing else;
# 4321290 (the CIFAR-10 generator): every lane takes eight two-vector trips, 31746 lanes a single vector behind them, tail of 2
OPT_N = [1, 3, 4, 5, 1000, ONE_TRIP + 3, ONE_TRIP + 4, 2 * ONE_TRIP, 4321290]
GUARD = 8               # NaN floats on either side of every buffer (a multiple of 4: the buffers stay 16-byte aligned)

LR = R.f32(2e-4)
MU, WD = R.f32(0.9), R.f32(0.01)
ALPHA, EPS = R.f32(0.99), R.f32(1e-8)
B1, B2 = R.f32(0.9), R.f32(0.999)


def _ops():
    from mcgen_amd import ops
    return ops


def _assert_within(got, ref, tol, what):
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    print(f'{what}: max error {float(err.max()):.3e}, max error / bound {float((err / tol.clamp_min(1e-300)).max()):.3f}')
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {err.numel()} outside the bound; first at flat index {i}: '
                             f'got {float(got.flatten()[i])}, ref {float(ref.flatten()[i])}, tol {float(tol.flatten()[i])}')


class _Guarded:
    """A device buffer of n floats between two NaN regions of `guard` floats."""

    def __init__(self, x, guard=GUARD):
        n = x.numel()
        full = torch.full((n + 2 * guard,), NAN)
        full[guard:guard + n] = x
        self.full = full.cuda()
        self.t = self.full[guard:guard + n]
        self.guard = guard

    def check(self, what):
        g = self.guard
        assert torch.isnan(self.full[:g]).all() and torch.isnan(self.full[-g:]).all(), f'{what}: a guard region was written'


def _grad_err(gi, wd):
    """g' = fma(wd, p, g): one rounding; exact when wd = 0."""
    return U32 * gi.abs() if wd != 0 else torch.zeros_like(gi)


def _sgd_tol(gi, buf2, p2, lr, mu, wd):
    """Bound on (p', buf') of one mcgen_sgd update.  3 roundings, one fma each: g' = fma(wd, p, g): dg = u |g'|;
    buf' = fma(mu, buf, g'): dbuf = dg + u |buf'|; p' = fma(-lr, s, p) with s = buf' (or g' when mu = 0): lr ds + u |p'|.
    All doubled."""
    ds = _grad_err(gi, wd)
    if mu != 0:
        ds = ds + U32 * buf2.abs()
    return 2 * (lr * ds + U32 * p2.abs()), 2 * ds


def _rmsprop_tol(gi, sq, sq2, buf2, p2, lr, alpha, eps, mu, wd):
    """Bound on (p', square_avg', buf') of one mcgen_rmsprop update.  g' as in _sgd_tol (1 rounding).
    sq' = fma(alpha, sq, ((1 - alpha) g') g'): 4 roundings (1 - alpha, two products, the fma):
    dsq = (1 - alpha)(2 |g'| dg + dg^2) + 4u ((1 - alpha) g'^2 + alpha sq).  r = sqrt(sq'): min(dsq / 2r, sqrt dsq) + u r.
    avg = r + eps: dr + u avg.  q = g' / avg (division: 2u): dq = dg / avg + |q| (davg / avg + 2u).
    buf' = fma(mu, buf, q): dbuf = dq + u |buf'|.  p' = fma(-lr, s, p), s = buf' or q: lr ds + u |p'|.  All doubled."""
    dg = _grad_err(gi, wd)
    dsq = (1 - alpha) * (2 * gi.abs() * dg + dg * dg) + 4 * U32 * ((1 - alpha) * gi * gi + alpha * sq.abs())
    r = sq2.clamp_min(0).sqrt()
    dr = torch.minimum(dsq / (2 * r).clamp_min(1e-300), dsq.sqrt()) + U32 * r
    avg = r + eps
    davg = dr + U32 * avg
    q = gi / avg
    ds = dg / avg + q.abs() * (davg / avg + 2 * U32)
    if mu != 0:
        ds = ds + U32 * buf2.abs()
    return 2 * (lr * ds + U32 * p2.abs()), 2 * dsq, 2 * ds


def _adamax_tol(gi, m, m2, u2, p2, t, lr, b1, b2, eps, wd):
    """Bound on (p', exp_avg', exp_inf') of one mcgen_adamax update.  g' as in _sgd_tol (1 rounding).
    m' = fma(b1, m, (1 - b1) g'): 3 roundings (1 - b1, the product, the fma): dm = (1 - b1) dg + 3u ((1 - b1)|g'| + b1 |m|).
    u' = max(b2 u, |g'| + eps): one rounding in either candidate, max is 1-Lipschitz: du = dg + u u'.
    clr = lr / bc1 with bc1 = 1 - b1^t rounded to fp32 (u) and the division (2u): 3u relative.
    q = m' / u' (2u): dq = dm / u' + |q| (du / u' + 2u).  p' = fma(-clr, q, p): clr dq + 3u |clr q| + u |p'|.  All doubled."""
    dg = _grad_err(gi, wd)
    dm = (1 - b1) * dg + 3 * U32 * ((1 - b1) * gi.abs() + b1 * m.abs())
    du = dg + U32 * u2
    clr = lr / (1 - b1 ** t)
    q = m2 / u2
    dq = dm / u2 + q.abs() * (du / u2 + 2 * U32)
    return 2 * (clr * dq + 3 * U32 * clr * q.abs() + U32 * p2.abs()), 2 * dm, 2 * du


def _gradient(n, gen):
    g = torch.randn(n, generator=gen)
    g[::7] = 0.0                  # exactly 0 and far below eps: from zero state RMSprop forms 0 / eps, Adamax m / u with u = eps
    g[1::7] = 1e-12
    return g


class _Case:
    """One optimizer's buffers, launch and reference for the kernel test."""

    def __init__(self, name, n, seeded, gen, guard=GUARD):
        self.name, self.seeded = name, seeded
        self.mu = MU if seeded else 0.0
        self.wd = WD if seeded else 0.0
        self.p = _Guarded(torch.randn(n, generator=gen) * 0.05, guard)
        zeros = torch.zeros(n)
        if name == 'sgd':
            init = {'buf': torch.randn(n, generator=gen) * 1e-2} if seeded else {}
        elif name == 'rmsprop':
            init = {'sq': torch.rand(n, generator=gen) * 1e-4 if seeded else zeros}
            if seeded:
                init['buf'] = torch.randn(n, generator=gen)
        else:
            init = {'m': torch.randn(n, generator=gen) * 1e-3 if seeded else zeros,
                    'u': torch.rand(n, generator=gen) * 1e-2 + 1e-6 if seeded else zeros}
        self.state = {k: _Guarded(v, guard) for k, v in init.items()}
        self.lr_arg = torch.tensor([LR], dtype=torch.float32, device='cuda') if seeded else LR

    def launch(self, g, step):
        ops, s = _ops(), {k: v.t for k, v in self.state.items()}
        if self.name == 'sgd':
            ops.sgd(self.p.t, g, s.get('buf'), step, self.lr_arg, self.mu, self.wd)
        elif self.name == 'rmsprop':
            ops.rmsprop(self.p.t, g, s['sq'], s.get('buf'), step, self.lr_arg, ALPHA, EPS, self.mu, self.wd)
        else:
            ops.adamax(self.p.t, g, s['m'], s['u'], step, self.lr_arg, (B1, B2), EPS, self.wd)

    def reference(self, p0, s0, g, t):
        """-> {name: (float64 reference, bound)} of one update from the kernel's own previous p and state."""
        mu, wd = self.mu, self.wd
        g = g.double()
        gi = g + wd * p0 if wd != 0 else g
        if self.name == 'sgd':
            p2, buf2 = OR.sgd(p0, g, s0.get('buf'), LR, mu, wd)
            tp, tb = _sgd_tol(gi, buf2, p2, LR, mu, wd)
            out = {'p': (p2, tp)}
            if mu != 0:
                out['buf'] = (buf2, tb)
        elif self.name == 'rmsprop':
            p2, sq2, buf2 = OR.rmsprop(p0, g, s0['sq'], s0.get('buf'), LR, ALPHA, EPS, mu, wd)
            tp, tsq, tb = _rmsprop_tol(gi, s0['sq'], sq2, buf2, p2, LR, ALPHA, EPS, mu, wd)
            out = {'p': (p2, tp), 'sq': (sq2, tsq)}
            if mu != 0:
                out['buf'] = (buf2, tb)
        else:
            p2, m2, u2 = OR.adamax(p0, g, s0['m'], s0['u'], t, LR, B1, B2, EPS, wd)
            tp, tm, tu = _adamax_tol(gi, s0['m'], m2, u2, p2, t, LR, B1, B2, EPS, wd)
            out = {'p': (p2, tp), 'm': (m2, tm), 'u': (u2, tu)}
        return out

    def run(self, gen, launches=3):
        n = self.p.t.numel()
        t0 = 10 ** 6 - 1 if self.seeded else 0
        step = torch.tensor([t0, 0], dtype=torch.int64, device='cuda')
        for k in range(launches):
            g = _Guarded(_gradient(n, gen), self.p.guard)
            p0 = self.p.t.cpu().double()
            s0 = {key: v.t.cpu().double() for key, v in self.state.items()}
            self.launch(g.t, step)
            torch.cuda.synchronize()
            t = t0 + k + 1
            assert step.tolist() == [t, 0], f'after launch {k + 1}: step {step.tolist()}'
            for key, (ref, tol) in self.reference(p0, s0, g.t.cpu(), t).items():
                got = self.p.t if key == 'p' else self.state[key].t
                assert torch.isfinite(got).all(), f'{self.name} n={n} t={t}: {key} is not finite'
                _assert_within(got, ref, tol, f'{self.name} n={n} t={t}: {key}')
            for key, buf in [('p', self.p), ('g', g)] + list(self.state.items()):
                buf.check(f'{self.name} n={n} t={t}: {key}')


@pytest.mark.parametrize('seeded', [False, True])
@pytest.mark.parametrize('n', OPT_N)
@pytest.mark.parametrize('name', ['sgd', 'rmsprop', 'adamax'])
def test_kernel_against_float64(name, n, seeded):
    """mcgen_sgd / mcgen_rmsprop / mcgen_adamax over three launches against float64, step by step (each step from the
    kernel's own p and state), to the bounds of _sgd_tol / _rmsprop_tol / _adamax_tol.  Unseeded: the counter from 0, zero
    state, lr as a float, no weight decay, momentum 0 (NULL buffer).  Seeded: the counter from 10^6 - 1, state from
    earlier steps, lr as a device tensor, weight decay 0.01, momentum 0.9.  One gradient in seven is exactly 0 and one in
    seven 1e-12; every result is finite.  After every launch the counter and its ticket read [t, 0], and the NaN guard
    regions around p, g and every state buffer are still NaN.  Sizes: see OPT_N."""
    gen = torch.Generator().manual_seed(n % 9973 + 2 * len(name) + seeded)
    _Case(name, n, seeded, gen).run(gen)


@pytest.mark.parametrize('name', ['sgd', 'rmsprop', 'adamax'])
def test_unaligned_buffers_take_the_scalar_loop(name):
    """Buffers that do not start on 16 bytes (guards of 5 floats) are walked by the scalar loop alone: same bounds."""
    gen = torch.Generator().manual_seed(77)
    _Case(name, 1001, True, gen, guard=5).run(gen, launches=1)


def test_arguments_are_checked():
    from mcgen_amd._lib import McgenError
    ops = _ops()
    p, g, s = (torch.zeros(8, device='cuda') for _ in range(3))
    step = torch.zeros(2, dtype=torch.int64, device='cuda')
    with pytest.raises(McgenError):
        ops.sgd(p, g, None, step, LR, 0.9, 0.0)              # momentum without a buffer
    with pytest.raises(McgenError):
        ops.sgd(p, g, s, step, LR, 0.0, 0.0)                 # a buffer without momentum
    with pytest.raises(McgenError):
        ops.rmsprop(p, g, s, None, step, LR, ALPHA, EPS, 0.9, 0.0)
    with pytest.raises(McgenError):
        ops.adamax(p[:0], g[:0], s[:0], s[:0], step, LR)     # n = 0
    torch.cuda.synchronize()
    assert step.tolist() == [0, 0] and float(p.abs().max()) == 0.0


# ---- trainers -----------------------------------------------------------------------------------------------------------
OPTIMIZERS = [('SGD', 0.9), ('RMSprop', 0.9), ('Adamax', 0.0)]
TRAIN_WD = 0.01


def _vae_model():
    from test_mcvae_gpu import _model
    return _model(gu.state_from_npz(gu.load_npz('mcvae_small.npz')))


def _vae_batch():
    d = gu.load_npz('mcvae_small.npz')
    return (torch.from_numpy(d['img']).cuda(), torch.from_numpy(d['label']).cuda(),
            [torch.from_numpy(d[f'noise/{s}/0']).cuda() for s in range(3)])


class _Float64Optimizer:
    """The float64 restatement with its own state from zero, and the bound of one step (the kernel test's)."""

    def __init__(self, name, n, lr, mu, wd, betas):
        self.name, self.lr, self.mu, self.wd, self.t = name, R.f32(lr), R.f32(mu), R.f32(wd), 0
        self.b1, self.b2 = R.f32(betas[0]), R.f32(betas[1])
        z = torch.zeros(n, dtype=torch.float64)
        self.s = {'SGD': [z if mu else None], 'RMSprop': [z, z if mu else None], 'Adamax': [z, z]}[name]

    def step(self, p0, g):
        """-> (p', bound on p') of one update from p0 with gradient g."""
        self.t += 1
        lr, mu, wd = self.lr, self.mu, self.wd
        gi = g + wd * p0 if wd != 0 else g
        if self.name == 'SGD':
            p2, buf2 = OR.sgd(p0, g, self.s[0], lr, mu, wd)
            self.s = [buf2]
            return p2, _sgd_tol(gi, buf2, p2, lr, mu, wd)[0]
        if self.name == 'RMSprop':
            sq = self.s[0]
            p2, sq2, buf2 = OR.rmsprop(p0, g, sq, self.s[1], lr, ALPHA, EPS, mu, wd)
            self.s = [sq2, buf2]
            return p2, _rmsprop_tol(gi, sq, sq2, buf2, p2, lr, ALPHA, EPS, mu, wd)[0]
        m = self.s[0]
        p2, m2, u2 = OR.adamax(p0, g, m, self.s[1], self.t, lr, self.b1, self.b2, EPS, wd)
        self.s = [m2, u2]
        return p2, _adamax_tol(gi, m, m2, u2, p2, self.t, lr, self.b1, self.b2, EPS, wd)[0]


@pytest.mark.parametrize('name,mu', OPTIMIZERS)
def test_vae_trainer_step_is_the_torch_update_of_its_gradient(name, mu):
    """VAETrainer(optimizer=name) on mcvae_small.npz, three eager iterations with the fixture's noise: each iteration's
    parameters equal the float64 restatement applied to the parameters before it and to tr.gflat, the clipped gradient the
    optimizer consumed, with the restatement's own float64 state carried from zero -- to the kernel test's bound, summed
    over the steps so far (the fp32 state's error of the earlier steps enters the later updates)."""
    from mcgen_amd.trainer import VAETrainer
    img, lab, eps = _vae_batch()
    tr = VAETrainer(_vae_model(), optimizer=name, momentum=mu, weight_decay=TRAIN_WD)
    assert type(tr.opt).__name__ == 'Fused' + name and tr.opt.lr == 3e-4
    ref = _Float64Optimizer(name, tr.fs.ensure().numel(), 3e-4, mu, TRAIN_WD, (0.9, 0.999))
    total = 0.0
    for s in range(3):
        p0 = tr.fs.ensure().cpu().double()
        loss = tr.train_iteration(img, lab, eps[s])
        assert torch.isfinite(loss)
        g = tr.gflat.cpu().double()
        assert float(g.abs().max()) > 0
        p2, tol = ref.step(p0, g)
        total = total + tol
        _assert_within(tr.fs.ensure(), p2, total, f'{name} step {s + 1}: parameters')
    assert int(tr.opt.step_count) == 3
    assert float((tr.fs.ensure().cpu().double() - p0).abs().max()) > 0


def _gan(optimizer=None, graphed=False, **k):
    from mcgen_amd import trainer as T
    from test_mcgan_gpu import _build
    d = gu.load_npz('mcgan_small.npz')
    m = _build([32] * 4, [16] * 4, 10, 'CIFAR10', gu.state_from_npz(d))
    cls = T.GraphedGANTrainer if graphed else T.GANTrainer
    tr = cls(m, 10, **(dict(k, optimizer=optimizer) if optimizer else k))
    img, lab = torch.from_numpy(d['img']).cuda(), torch.from_numpy(d['label']).cuda()
    return tr, img, lab, [torch.from_numpy(z).cuda() for z in d['z']]


@pytest.mark.parametrize('name,mu', OPTIMIZERS)
def test_discriminator_update_takes_the_unfused_route(name, mu):
    """One discriminator update of the small MCGAN with a non-Adam optimizer: d_compute, then d_apply equals the float64
    restatement on grad_d (the spectral-norm-fixed gradient) to the kernel test's bound.  Then a whole d_update: no raw
    gradients are left pending for the Adam-only fused launch, and the parameters again follow grad_d."""
    tr, img, lab, zs = _gan(name, momentum=mu, weight_decay=TRAIN_WD)
    assert type(tr.opt_d).__name__ == type(tr.opt_g).__name__ == 'Fused' + name and not tr._fuse_d
    tr.model.train(True)
    n = img.shape[0]
    ind, ind2, _ = tr.indicators(lab, 1)
    ref = _Float64Optimizer(name, tr.deng.flat_p.ensure().numel(), 2e-4, mu, TRAIN_WD, (0.5, 0.999))
    total = 0.0
    for k in range(2):
        fake = tr.g_fakes(ind, zs[k], 1)
        tr.grad_d.zero_()                                       # the update must come from what this pass writes
        if k == 0:
            tr.d_compute(img, ind, fake, ind2)
            p0 = tr.deng.flat_p.ensure().cpu().double()
            tr.d_apply()
        else:
            p0 = tr.deng.flat_p.ensure().cpu().double()
            tr.d_update(img, ind, fake, ind2)
        assert tr.deng.pending_fix is None
        g = tr.grad_d.cpu().double()
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0
        p2, tol = ref.step(p0, g)
        total = total + tol
        _assert_within(tr.deng.flat_p.ensure(), p2, total, f'{name} D update {k + 1}: parameters')
    assert int(tr.opt_d.step_count) == 2 and int(tr.opt_g.step_count) == 0
    # the default trainer keeps the fused spectral-norm fix + Adam launch
    from mcgen_amd.trainer import _FUSE_D_ADAM
    assert _gan()[0]._fuse_d == _FUSE_D_ADAM


# ---- replay -------------------------------------------------------------------------------------------------------------
def test_vae_replay_with_sgd_momentum_matches_eager():
    """test_replay_follows_a_learning_rate_change_without_recapture with FusedSGD (momentum 0.9): eager and graph replay
    agree over three iterations to that test's tolerances while the rate changes between replays without a re-capture
    (capture left the momentum buffer and the counter as they were); a changed momentum refuses to replay."""
    from mcgen_amd.trainer import VAETrainer
    img, lab, eps = _vae_batch()
    te, tg = (VAETrainer(_vae_model(), optimizer='SGD', momentum=0.9) for _ in range(2))
    tg.capture(img, lab, warmup=1)
    assert int(tg.opt.step_count) == 0 and float(tg.opt.buf.abs().max()) == 0.0
    key = tg._hyper_key
    rates = [3e-4, 1.5e-4, 6e-4]
    for s in range(3):
        te.opt.set_lr(rates[s]); tg.opt.set_lr(rates[s])
        le, lg = te.train_iteration(img, lab, eps[s]), tg.train_iteration(img, lab, eps[s])
        assert abs(float(le) - float(lg)) < 1e-6 * (1 + abs(float(le))), (s, float(le), float(lg))
    assert tg._hyper_key == key and tg.opt.state_dict()['param_groups'][0]['lr'] == 6e-4 and int(tg.opt.step_count) == 3
    for (k, a), (_, b) in zip(te.model.state_dict().items(), tg.model.state_dict().items()):
        assert float((a.float() - b.float()).abs().max()) <= 1e-6 * (1 + float(a.float().abs().max())), k
    # the rate really is applied: a third trainer that never changes it ends elsewhere
    t0 = VAETrainer(_vae_model(), optimizer='SGD', momentum=0.9)
    for s in range(3):
        t0.train_iteration(img, lab, eps[s])
    assert float((t0.fs.ensure() - tg.fs.ensure()).abs().max()) > 1e-7
    tg.opt.momentum = 0.5
    with pytest.raises(RuntimeError):
        tg.train_iteration(img, lab, eps[0])


def test_graphed_gan_with_rmsprop_matches_eager():
    """test_graphed_trainer_matches_eager with RMSprop on both networks: capture leaves model and optimizer state
    untouched, three replayed iterations with the fixture's latents land on the eager trainer's state (that test's
    tolerances) while the rate changes between replays without a re-capture; a changed momentum is not replayed from the
    stale graph (GraphedGANTrainer captures again, as it does for a changed beta)."""
    tr, img, lab, zs = _gan('RMSprop', graphed=True)
    sd0 = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items()}
    tr.capture(img, lab, warmup=1)
    torch.cuda.synchronize()
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v.cpu(), sd0[k]), k
    for o in (tr.opt_g, tr.opt_d):
        assert int(o.step_count) == 0 and float(o.sq.abs().max()) == 0.0 and o.buf is None
    te = _gan('RMSprop')[0]
    captured = lambda: tr.g_all if tr.g_all is not None else tr.g_ga      # (one graph, or one per phase)
    graph, key = captured(), tr._hyper_key
    rates = [2e-4, 1e-4, 4e-4]
    for it in range(3):
        for t in (tr, te):
            t.opt_g.set_lr(rates[it]); t.opt_d.set_lr(rates[it])
        dl, gl = tr.train_iteration(img, lab, zs[6 * it:6 * it + 6])
        de, ge = te.train_iteration(img, lab, zs[6 * it:6 * it + 6])
        assert torch.isfinite(dl) and torch.isfinite(gl)
        atol = 1e-4 if it == 0 else 2e-3                        # (that test's bounds on the losses)
        assert abs(float(dl) - float(de)) <= atol and abs(float(gl) - float(ge)) <= atol, (it, float(dl), float(de), float(gl), float(ge))
    assert captured() is graph and tr._hyper_key == key
    sd_g, sd_e = tr.model.state_dict(), te.model.state_dict()
    for k, v in sd_e.items():
        if v.dtype == torch.int64:
            assert int(sd_g[k]) == int(v), k
        else:
            assert float((sd_g[k] - v).abs().max()) <= 1e-6 + 1e-5 * float(v.abs().max()), k
    assert int(tr.opt_d.step_count) == 15 and int(tr.opt_g.step_count) == 3
    tr.opt_d.momentum = 0.9
    tr.train_iteration(img, lab, zs[:6])
    assert tr._hyper_key != key and captured() is not graph and tr.opt_d.buf is not None
    assert int(tr.opt_d.step_count) == 20


# ---- resume -------------------------------------------------------------------------------------------------------------
def test_resume_with_rmsprop_momentum_is_bit_exact(tmp_path):
    """Two eager iterations with FusedRMSprop (momentum 0.9), a checkpoint through checkpoint.make_checkpoint (the state
    travels as torch.optim.RMSprop's), a fresh model and trainer, a third iteration: the parameters equal the
    uninterrupted run's bit for bit."""
    from mcgen_amd import checkpoint as ck
    from mcgen_amd.trainer import VAETrainer
    img, lab, eps = _vae_batch()
    kw = dict(optimizer='RMSprop', momentum=0.9, weight_decay=TRAIN_WD)
    tr = VAETrainer(_vae_model(), **kw)
    for s in range(2):
        tr.train_iteration(img, lab, eps[s])
    path = str(tmp_path / 'ck.pt')
    ck.save(ck.make_checkpoint(tr.model, tr.opt, 3), path)
    tr.train_iteration(img, lab, eps[2])
    raw = ck.load(path)
    assert set(raw['optimizer_dict']['state'][0]) == {'step', 'square_avg', 'momentum_buffer'}
    assert raw['optimizer_dict']['param_groups'][0]['momentum'] == 0.9
    t2 = VAETrainer(_vae_model(), optimizer='RMSprop')           # momentum arrives with the state
    epoch, _ = ck.resume(path, t2.model, t2.opt)
    assert epoch == 3 and int(t2.opt.step_count) == 2 and t2.opt.hyper() == tr.opt.hyper()
    torch.optim.RMSprop(t2.model.parameters()).load_state_dict(raw['optimizer_dict'])     # a reference-side resume reads it
    t2.train_iteration(img, lab, eps[2])
    worst = max(float((a.float() - b.float()).abs().max()) for a, b in zip(tr.model.state_dict().values(), t2.model.state_dict().values()))
    print(f'largest difference between the resumed and the uninterrupted run: {worst:.3e}')
    for (k, a), (_, b) in zip(tr.model.state_dict().items(), t2.model.state_dict().items()):
        assert torch.equal(a, b), k
