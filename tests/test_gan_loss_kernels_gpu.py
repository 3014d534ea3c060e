"""The loss-typed kernels of csrc/small_ops.hip (cfg['loss_type'], train_gan.py:148-156,168-174), one at a time:
mcgen_gan_loss_d / mcgen_gan_loss_g, mcgen_dtail_loss_fused and mcgen_dtail_pair_wgrad_gan_loss.  Conventions and helpers are
those of test_mcgan_tail_code_ops_gpu.py: NaN-gapped output buffers, float64 references on the CPU from exactly the values
the kernel read, a device error ends the session.  No bound is measured on the code under test:

- the BCE gradients and losses: tests/gan_loss_ref.py's module docstring (sigmoid within 5u, softplus within
  (3 + 2 LOG1P_ULP) u, TINY where expf overflows or a result is subnormal, doubled for second-order terms).  There is no
  decision threshold: every sample of every case is compared.
- the fused tail: pooled and logit to small_ops_ref.tail_bounds; dlogit against float64 applied to the logit the kernel
  itself wrote (an fp32 number, so the reference is exact in its input); dx to the tail's own 5u (+ 2^-8 in bf16) of the
  float64 product formed from the dlogit the kernel wrote.
- MCGEN_GAN_LOSS_HINGE through a new entry equals the hinge entry bit for bit (NaN-gapped buffers compared as words), and
  the BCE derivative of the fused launch equals the stand-alone kernel's on the same logits bit for bit, as its loss value
  in the paired weight-gradient launch equals mcgen_gan_loss_d's.
"""
import pytest
import torch

import gan_loss_ref as G
import small_ops_ref as R
import test_mcgan_tail_code_ops_gpu as T
from test_mcgan_tail_code_ops_gpu import _assert_within, _dev, _dt, _dtc, _lib, _nan, _ok, _out, _p, _stream

pytestmark = pytest.mark.gpu

U32 = G.U32
HINGE, BCE = 0, 1


def _same_words(a, b, what):
    """Two NaN-gapped fp32 / bf16 buffers hold the same bits (NaN gaps included)."""
    assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                       b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)), f'{what}: bits differ'


def _loss_d(real_dev, fake_dev, n, lt):
    loss, dr, df = _nan(1), _nan(n), _nan(n)
    _ok(_lib().mcgen_gan_loss_d(_p(real_dev), _p(fake_dev), n, lt, _p(loss), _p(dr), _p(df), _stream()), 'gan_loss_d')
    return loss, dr, df


def _loss_g(fake_dev, n, lt):
    loss, df = _nan(1), _nan(n)
    _ok(_lib().mcgen_gan_loss_g(_p(fake_dev), n, lt, _p(loss), _p(df), _stream()), 'gan_loss_g')
    return loss, df


def _check_grad(got, ref, x, n, sign, what):
    """`got` [N] against the float64 gradient `ref` of the logits x: the bound, finiteness, and +-0.5 / N to 2u at x = 0."""
    assert bool(torch.isfinite(got).all()), f'{what}: a non-finite gradient'
    _assert_within(got, ref, G.grad_tol(ref), what)
    zero = x.double() == 0
    if bool(zero.any()):
        half = sign * 0.5 / n
        assert bool(((got[zero] - half).abs() <= 2 * U32 * abs(half)).all()), f'{what}: the gradient at an exact 0 logit'


# ---- 1. the stand-alone losses --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 1000])
def test_bce_losses(n):
    """mcgen_gan_loss_d / mcgen_gan_loss_g with BCE: one block of 256 threads (N = 257: a second trip of the stride loop, 255:
    an idle lane); random logits with 0, +-1, +-17, +-88.8, +-100.5, +-200 at both ends (N = 1, 2: every extreme in turn)."""
    k = len(G.EXTREMES)
    if n < k:
        e = torch.tensor(G.EXTREMES)
        cases = [(e.roll(i)[:n].clone(), e.roll(i + 3)[:n].clone()) for i in range(k)]
    else:
        cases = [(G.logits_with_extremes(n, 'real'), G.logits_with_extremes(n, 'fake').flip(0))]
    for real, fake in cases:
        loss, dr, df = _loss_d(_dev(real), _dev(fake), n, BCE)
        lref, drr, dfr, _ = G.bce_d(real, fake)
        _check_grad(_out(dr, n, 'dreal'), drr, real, n, -1, f'bce_d dreal, N = {n}')
        _check_grad(_out(df, n, 'dfake'), dfr, fake, n, +1, f'bce_d dfake, N = {n}')
        got = _out(loss, 1, 'loss')
        assert bool(torch.isfinite(got).all())
        _assert_within(got, lref.view(1), G.loss_tol(torch.cat([G.softplus(-real), G.softplus(fake)]), n), f'bce_d loss, N = {n}')
        loss, df = _loss_g(_dev(fake), n, BCE)
        lref, dfr, _ = G.bce_g(fake)
        _check_grad(_out(df, n, 'dfake'), dfr, fake, n, -1, f'bce_g dfake, N = {n}')
        got = _out(loss, 1, 'loss')
        assert bool(torch.isfinite(got).all())
        _assert_within(got, lref.view(1), G.loss_tol(G.softplus(-fake), n), f'bce_g loss, N = {n}')


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 1000])
def test_hinge_through_the_loss_typed_entries_is_the_hinge_kernels(n):
    lib = _lib()
    real, fake = G.logits_with_extremes(n, 'real'), G.logits_with_extremes(n, 'fake').flip(0)
    rd, fd = _dev(real), _dev(fake)
    new = _loss_d(rd, fd, n, HINGE)
    old = [_nan(1), _nan(n), _nan(n)]
    _ok(lib.mcgen_hinge_d(_p(rd), _p(fd), n, *[_p(o) for o in old], _stream()), 'hinge_d')
    for a, b, what in zip(new, old, ('loss', 'dreal', 'dfake')):
        _same_words(a, b, f'hinge d {what}')
    new = _loss_g(fd, n, HINGE)
    old = [_nan(1), _nan(n)]
    _ok(lib.mcgen_hinge_g(_p(fd), n, *[_p(o) for o in old], _stream()), 'hinge_g')
    for a, b, what in zip(new, old, ('loss', 'dfake')):
        _same_words(a, b, f'hinge g {what}')


# ---- 2. the fused tail ------------------------------------------------------------------------------------------------------
# C = 8: all 256 pixel lanes; C = 40: a ragged lane split (6 lanes of 5 groups, 16 threads idle); C = 2048: one lane row;
# N = 258: more than 256 workgroups, halves of 129 samples
PAIR_SHAPES = [(2, 40, 5), (6, 8, 16), (4, 2048, 1), (258, 128, 4)]
G_SHAPES = PAIR_SHAPES + [(1, 40, 5), (5, 8, 16)]
FUSED_CASES = [(s, 'd_pair') for s in PAIR_SHAPES] + [(s, 'g') for s in G_SHAPES]


def _launch_loss_fused(d, shape, bf16, mode, lt):
    """mcgen_dtail_loss_fused on the device inputs d -> the four NaN-gapped buffers (pooled, logit, dlogit, dx)."""
    n, c, hw = shape
    outs = [_nan(n * c), _nan(n), _nan(n), _nan(n * hw * c, _dt(bf16))]
    _ok(_lib().mcgen_dtail_loss_fused(_p(d['x']), _dtc(bf16), _p(d['code']), _p(d['w']), _p(d['b']), _p(d['sigma']),
                                      *[_p(o) for o in outs], n, hw, c, {'d_pair': 0, 'g': 1}[mode], lt, _stream()), 'dtail_loss_fused')
    return outs


def _spread_logits(t):
    """Scale w and b so that the logits cover the sigmoid's range, saturated samples included."""
    t['w'] = t['w'] * 6.0
    t['b'] = t['b'] * 4.0
    return t


@pytest.mark.parametrize('with_code', [True, False])
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('shape,mode', FUSED_CASES)
def test_fused_tail_bce(shape, mode, bf16, with_code):
    n, c, hw = shape
    t = _spread_logits(R.tail_inputs(n, c, hw, bf16, with_code, 'bce', mode))
    what = f'fused bce {shape} {mode} bf16={bf16} code={with_code}'
    d = {k: (_dev(v.to(_dt(bf16))) if k == 'x' else _dev(v)) for k, v in t.items()}
    b_pooled, b_logit, b_dlogit, b_dx = _launch_loss_fused(d, shape, bf16, mode, BCE)
    pooled, logit = _out(b_pooled, n * c, 'pooled').view(n, c), _out(b_logit, n, 'logit')
    dlogit, dx = _out(b_dlogit, n, 'dlogit'), _out(b_dx, n * hw * c, 'dx').view(n, hw, c)
    ref = R.dtail(t['x'], t['code'], t['w'], t['b'], t['sigma'])
    tol_p, tol_l = R.tail_bounds(t, ref)
    _assert_within(pooled, ref['pooled'], tol_p, f'{what}: pooled')
    _assert_within(logit, ref['logit'], tol_l, f'{what}: logit')
    # d loss / d logit in float64 from the logit the kernel wrote: every sample, no threshold
    if mode == 'g':
        dref = G.bce_g(logit)[1]
    else:
        h = n // 2
        _, dr, df, _ = G.bce_d(logit[:h], logit[h:])
        dref = torch.cat([dr, df])
        assert bool((dlogit[:h] <= 0).all()) and bool((dlogit[h:] >= 0).all())
    assert bool(torch.isfinite(dlogit).all())
    _assert_within(dlogit, dref, G.grad_tol(dref), f'{what}: dlogit')
    dxref, mask = R.dtail_dx(dlogit, t['x'], t['code'], t['w'], t['sigma'])
    _assert_within(dx, dxref, T._dx_tol(dxref, mask, bf16), f'{what}: dx')
    assert bool((dx[t['x'] == 0] == 0).all())
    # the stand-alone loss kernel on the fused launch's logits writes the same derivative, bit for bit
    if mode == 'g':
        _, alone = _loss_g(b_logit, n, BCE)
        assert torch.equal(alone[:n].view(torch.int32), b_dlogit[:n].view(torch.int32)), f'{what}: gan_loss_g differs'
    else:
        _, a_r, a_f = _loss_d(b_logit, b_logit[h:], h, BCE)
        assert torch.equal(torch.cat([a_r[:h], a_f[:h]]).view(torch.int32), b_dlogit[:n].view(torch.int32)), f'{what}: gan_loss_d differs'
    # HINGE through the new entry: every output is mcgen_dtail_hinge_fused's, bit for bit
    new = _launch_loss_fused(d, shape, bf16, mode, HINGE)
    old = [_nan(n * c), _nan(n), _nan(n), _nan(n * hw * c, _dt(bf16))]
    _ok(_lib().mcgen_dtail_hinge_fused(_p(d['x']), _dtc(bf16), _p(d['code']), _p(d['w']), _p(d['b']), _p(d['sigma']),
                                       *[_p(o) for o in old], n, hw, c, {'d_pair': 0, 'g': 1}[mode], _stream()), 'dtail_hinge_fused')
    for a, b, name in zip(new, old, ('pooled', 'logit', 'dlogit', 'dx')):
        _same_words(a, b, f'{what}: hinge {name}')
    # and the BCE launch's forward half is the hinge launch's
    _same_words(b_pooled, old[0], f'{what}: pooled vs the hinge launch')
    _same_words(b_logit, old[1], f'{what}: logit vs the hinge launch')


def test_fused_tail_bce_saturated_logits():
    """Logits driven to about +-200 and +-120 through the bias (every one past +-88.8, asserted on the reference): expf
    overflows, the derivative is 0 or -+1 / count, never NaN or inf, and dx is finite."""
    n, c, hw = 4, 8, 3
    for bias in (200.0, -200.0, 120.0, -120.0):
        t = R.tail_inputs(n, c, hw, False, False, 'sat')
        t['b'] = torch.tensor([bias])
        assert bool((R.dtail(t['x'], t['code'], t['w'], t['b'], t['sigma'])['logit'].abs() > 100).all())
        d = {k: _dev(v) for k, v in t.items()}
        for mode in ('d_pair', 'g'):
            _, b_logit, b_dlogit, b_dx = _launch_loss_fused(d, (n, c, hw), False, mode, BCE)
            logit, dlogit = _out(b_logit, n, 'logit'), _out(b_dlogit, n, 'dlogit')
            assert bool((logit.abs() > 88.8).all())
            dref = G.bce_g(logit)[1] if mode == 'g' else torch.cat(G.bce_d(logit[:2], logit[2:])[1:3])
            assert bool(torch.isfinite(dlogit).all()) and bool(torch.isfinite(_out(b_dx, n * hw * c, 'dx')).all())
            _assert_within(dlogit, dref, G.grad_tol(dref), f'saturated {bias} {mode}')


# ---- 3. the paired weight-gradient launch with the loss value ------------------------------------------------------------
@pytest.mark.parametrize('c', [8, 72])
@pytest.mark.parametrize('n', [1, 3, 257])
def test_pair_wgrad_gan_loss(n, c):
    """mcgen_dtail_pair_wgrad_gan_loss: dw1 / db1 / dw2 / db2 are mcgen_dtail_pair_wgrad's bit for bit for either loss, the
    BCE loss value is mcgen_gan_loss_d's on the same 2N logits bit for bit (and so within its bound), the hinge value
    mcgen_dtail_pair_wgrad_loss's."""
    lib = _lib()
    gen = T._gen('pair-gan-loss', n, c)
    dlogit = torch.randn(2 * n, generator=gen)
    pooled = torch.randn(2 * n, c, generator=gen).abs() * (torch.rand(2 * n, c, generator=gen) < 0.7)
    logit = torch.cat([G.logits_with_extremes(n, 'pr'), G.logits_with_extremes(n, 'pf').flip(0)])
    dl_d, pl_d, rt_d, lg_d = _dev(dlogit), _dev(pooled), _dev(torch.tensor([1.25])), _dev(logit)
    plain = [_nan(c), _nan(1), _nan(c), _nan(1)]
    _ok(lib.mcgen_dtail_pair_wgrad(_p(dl_d), _p(pl_d), _p(rt_d), n, c, *[_p(b) for b in plain], _stream()), 'dtail_pair_wgrad')
    for lt in (BCE, HINGE):
        outs, loss = [_nan(c), _nan(1), _nan(c), _nan(1)], _nan(1)
        _ok(lib.mcgen_dtail_pair_wgrad_gan_loss(_p(dl_d), _p(pl_d), _p(rt_d), _p(lg_d), n, c, *[_p(b) for b in outs], _p(loss), lt,
                                                _stream()), 'dtail_pair_wgrad_gan_loss')
        for a, b, name in zip(outs, plain, ('dw1', 'db1', 'dw2', 'db2')):
            _same_words(a, b, f'loss_type {lt}: {name}')
        alone, _, _ = _loss_d(lg_d, lg_d[n:], n, lt)
        _same_words(loss, alone, f'loss_type {lt}: the loss value vs mcgen_gan_loss_d')
        if lt == HINGE:
            old_outs, old = [_nan(c), _nan(1), _nan(c), _nan(1)], _nan(1)
            _ok(lib.mcgen_dtail_pair_wgrad_loss(_p(dl_d), _p(pl_d), _p(rt_d), _p(lg_d), n, c, *[_p(b) for b in old_outs], _p(old),
                                                _stream()), 'dtail_pair_wgrad_loss')
            _same_words(loss, old, 'hinge: the loss value vs mcgen_dtail_pair_wgrad_loss')
        else:
            lref = G.bce_d(logit[:n], logit[n:])[0]
            got = _out(loss, 1, 'loss')
            assert bool(torch.isfinite(got).all())
            _assert_within(got, lref.view(1), G.loss_tol(torch.cat([G.softplus(-logit[:n]), G.softplus(logit[n:])]), n), 'pair bce loss')
