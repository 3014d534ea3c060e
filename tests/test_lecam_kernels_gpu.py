"""The three kernel entries of the LeCam regulariser (csrc/small_ops.hip), one at a time, against tests/lecam_ref.py's
float64 references within its derived bounds: mcgen_lecam_loss_d, mcgen_dtail_lecam_fused and
mcgen_dtail_pair_wgrad_lecam_loss.  Conventions and helpers are those of test_gan_loss_kernels_gpu.py: NaN-gapped output
buffers, references computed from exactly the fp32 values the kernel read (dlogit from the logit the kernel itself wrote, so
the tail's matmul error does not enter), a device error ends the session.  No bound is measured on the code under test.

Bit-for-bit identities: an inactive term (lambda = 0, or t < start) gives the existing entries' outputs; the fused tail's
dlogit is the stand-alone entry's; the paired launch's loss value and new state are the stand-alone entry's; a second
launch on the same inputs and the same restored state repeats the first.  A refused call leaves state and outputs alone."""
import pytest
import torch

import gan_loss_ref as G
import lecam_ref as L
import small_ops_ref as R
import test_mcgan_tail_code_ops_gpu as T
from test_gan_loss_kernels_gpu import _launch_loss_fused, _loss_d, _same_words, _spread_logits
from test_mcgan_tail_code_ops_gpu import _assert_within, _dev, _dt, _dtc, _lib, _nan, _ok, _out, _p, _refused, _stream

pytestmark = pytest.mark.gpu

LOSSES = ['Hinge', 'BCE']
# dx = dlogit w / sigma code is three products; where a saturated sigmoid makes dlogit (and so dx) subnormal, each product
# and the store round to the subnormal spacing (fp32: 2^-149; a bf16 store: 2^-133) instead of relatively: 4 spacings
# (bf16: 3 and the store's) on top of the tail's 5u
SUB = {False: 4 * 2.0 ** -149, True: 3 * 2.0 ** -149 + 2.0 ** -133}
DECAY = 0.9


def _state_dev(state):
    """{'a_R', 'a_F', 't'} -> a mcgen_lecam_state_t on the device (int64[4]); the statistics start as NaN: whoever owes
    them must write them, whoever does not must leave them."""
    host = torch.zeros(4, dtype=torch.int64)
    f = host.view(torch.float32)
    f[0], f[1] = state['a_R'], state['a_F']
    f[2:6] = float('nan')
    host[3] = state['t']
    return host.cuda()


def _state_host(dev):
    h = dev.cpu()
    f = h.view(torch.float32).double()
    return {'a_R': float(f[0]), 'a_F': float(f[1]), 'm_R': float(f[2]), 'm_F': float(f[3]), 'r_t': float(f[4]), 'R': float(f[5]),
            't': int(h[3])}


def _lecam_d(real_dev, fake_dev, n, loss_type, st_dev, lam, decay, start):
    loss, dr, df = _nan(1), _nan(n), _nan(n)
    _ok(_lib().mcgen_lecam_loss_d(_p(real_dev), _p(fake_dev), n, L.LOSS_IDS[loss_type], _p(st_dev), lam, decay, start,
                                  _p(loss), _p(dr), _p(df), _stream()), 'lecam_loss_d')
    return loss, dr, df


def _check_state(got, ref, before, what):
    """The state the kernel left against the reference: t exactly, statistics and anchors within their bounds."""
    assert got['t'] == before['t'] + 1 == ref['state']['t'], f'{what}: t'
    for k in ('m_R', 'm_F', 'r_t'):
        assert abs(got[k] - float(ref['stats'][k])) <= float(ref['stats_tol'][k]), f'{what}: {k} {got[k]} vs {float(ref["stats"][k])}'
    assert abs(got['R'] - float(ref['R'])) <= float(ref['R_tol']), f'{what}: R {got["R"]} vs {float(ref["R"])}'
    for k in ('a_R', 'a_F'):
        assert abs(got[k] - ref['state'][k]) <= ref['anchor_tol'][k], f'{what}: {k} {got[k]} vs {ref["state"][k]}'


def _logits(n, *key):
    """gan_loss_ref.logits_with_extremes with +-1e4 added behind the extremes (N large enough) or in turn (small N)."""
    x = G.logits_with_extremes(n, *key)
    k = len(G.EXTREMES)
    if n >= 2 * k + 2:
        x[k], x[-k - 1] = 1e4, -1e4
    elif n >= 2:
        x[0], x[-1] = 1e4, -1e4
    else:
        x[0] = 1e4 if key[-1] == 'real' else -1e4
    return x


# ---- 1. the stand-alone entry ---------------------------------------------------------------------------------------------
ANCHORS = [(0.0, 0.0), (0.5, -0.5), (-0.5, 0.5), (50.0, -50.0), (-50.0, 50.0)]
# t = 0: the copy branch (and, with start = 0, an active term on zero or preset anchors); start - 1: the last inactive
# update; start: the first active one
STATE_CASES = [(0, 0), (0, 3), (2, 3), (3, 3), (7, 3)]


@pytest.mark.parametrize('loss_type', LOSSES)
@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
def test_lecam_loss_d(n, loss_type):
    """One block of 256 threads (257: a second trip of the stride loop; 255: an idle lane; 1000: four trips); logits with
    0, +-1, +-17, +-88.8, +-100.5, +-200 and +-1e4; every anchor pair against every state case."""
    real, fake = _logits(n, 'real'), _logits(n, 'fake').flip(0)
    rd, fd = _dev(real), _dev(fake)
    lam = 0.3
    for a_r, a_f in ANCHORS:
        for t, start in STATE_CASES:
            before = {'a_R': a_r, 'a_F': a_f, 't': t}
            what = f'lecam_loss_d {loss_type} N={n} anchors=({a_r}, {a_f}) t={t} start={start}'
            st = _state_dev(before)
            loss, dr, df = _lecam_d(rd, fd, n, loss_type, st, lam, DECAY, start)
            ref = L.lecam_d(real, fake, loss_type, before, lam, DECAY, start)
            assert ref['active'] == (t >= start)
            got_r, got_f, got_l = _out(dr, n, 'dreal'), _out(df, n, 'dfake'), _out(loss, 1, 'loss')
            assert bool(torch.isfinite(got_r).all()) and bool(torch.isfinite(got_f).all()) and bool(torch.isfinite(got_l).all())
            _assert_within(got_r, ref['dreal'], ref['dreal_tol'], f'{what}: dreal')
            _assert_within(got_f, ref['dfake'], ref['dfake_tol'], f'{what}: dfake')
            _assert_within(got_l, ref['loss'].view(1), ref['loss_tol'], f'{what}: loss')
            after = _state_host(st)
            _check_state(after, ref, before, what)
            if not ref['active']:
                # an inactive term: the existing entry's bits, loss value included
                old = _loss_d(rd, fd, n, L.LOSS_IDS[loss_type])
                for a, b, name in zip((loss, dr, df), old, ('loss', 'dreal', 'dfake')):
                    _same_words(a, b, f'{what}: inactive {name} vs mcgen_gan_loss_d')
            # the same inputs on the same restored state: the same bits
            st2 = _state_dev(before)
            again = _lecam_d(rd, fd, n, loss_type, st2, lam, DECAY, start)
            for a, b, name in zip((loss, dr, df), again, ('loss', 'dreal', 'dfake')):
                _same_words(a, b, f'{what}: second launch {name}')
            assert torch.equal(st, st2), f'{what}: second launch state'


def test_lecam_loss_d_lambda_zero_moves_the_state_only():
    """lambda = 0 through the entry: mcgen_gan_loss_d's bits, and the state moves (the caller decides whether to call)."""
    n = 300
    real, fake = _logits(n, 'real'), _logits(n, 'fake').flip(0)
    rd, fd = _dev(real), _dev(fake)
    for loss_type in LOSSES:
        before = {'a_R': 0.5, 'a_F': -0.5, 't': 4}
        st = _state_dev(before)
        new = _lecam_d(rd, fd, n, loss_type, st, 0.0, DECAY, 0)
        old = _loss_d(rd, fd, n, L.LOSS_IDS[loss_type])
        for a, b, name in zip(new, old, ('loss', 'dreal', 'dfake')):
            _same_words(a, b, f'{loss_type} lambda = 0: {name}')
        _check_state(_state_host(st), L.lecam_d(real, fake, loss_type, before, 0.0, DECAY, 0), before, f'{loss_type} lambda = 0')


def test_sign_statistic_counts_zero_as_zero():
    real = torch.tensor([0.0, -0.0, 2.0, -3.0, 5.0, 0.0, 1e-30, -1e-30])
    fake = torch.zeros(8)
    st = _state_dev(L.fresh_state())
    _lecam_d(_dev(real), _dev(fake), 8, 'Hinge', st, 0.3, DECAY, 0)
    got = _state_host(st)
    assert got['r_t'] == (2 - 1 + 1 - 1) / 8 and got['m_F'] == 0.0 and got['a_F'] == 0.0 and got['t'] == 1


# ---- 2. the fused tail ------------------------------------------------------------------------------------------------------
# C = 8: all 256 pixel lanes; C = 24: 256 does not divide by C / 8 = 3 (85 lanes, one thread idle); C = 2048: one lane row
TAIL_SHAPES = [(n, c, hw) for n in (2, 6) for c in (8, 24, 2048) for hw in (1, 16, 17)]
TAIL_STATES = [({'a_R': 0.0, 'a_F': 0.0, 't': 0}, 0), ({'a_R': 0.3, 'a_F': -0.2, 't': 2}, 3), ({'a_R': 0.3, 'a_F': -0.2, 't': 3}, 3),
               ({'a_R': -50.0, 'a_F': 50.0, 't': 9}, 0)]


def _launch_lecam_fused(d, shape, bf16, loss_type, st_dev, lam, start):
    n, c, hw = shape
    outs = [_nan(n * c), _nan(n), _nan(n), _nan(n * hw * c, _dt(bf16))]
    _ok(_lib().mcgen_dtail_lecam_fused(_p(d['x']), _dtc(bf16), _p(d['code']), _p(d['w']), _p(d['b']), _p(d['sigma']),
                                       *[_p(o) for o in outs], n, hw, c, L.LOSS_IDS[loss_type], _p(st_dev), lam, start, _stream()),
        'dtail_lecam_fused')
    return outs


@pytest.mark.parametrize('loss_type', LOSSES)
@pytest.mark.parametrize('with_code', [True, False])
@pytest.mark.parametrize('bf16', [False, True])
def test_fused_tail_lecam(bf16, with_code, loss_type):
    lam = 0.3
    for shape in TAIL_SHAPES:
        n, c, hw = shape
        h = n // 2
        t = _spread_logits(R.tail_inputs(n, c, hw, bf16, with_code, 'lecam'))
        d = {k: (_dev(v.to(_dt(bf16))) if k == 'x' else _dev(v)) for k, v in t.items()}
        tref = R.dtail(t['x'], t['code'], t['w'], t['b'], t['sigma'])
        tol_p, tol_l = R.tail_bounds(t, tref)
        plain = _launch_loss_fused(d, shape, bf16, 'd_pair', L.LOSS_IDS[loss_type])
        for before, start in TAIL_STATES:
            what = f'fused lecam {loss_type} {shape} bf16={bf16} code={with_code} t={before["t"]} start={start}'
            st = _state_dev(before)
            keep = st.clone()
            b_pooled, b_logit, b_dlogit, b_dx = _launch_lecam_fused(d, shape, bf16, loss_type, st, lam, start)
            assert torch.equal(st.view(torch.int32), keep.view(torch.int32)), f'{what}: the tail launch wrote the state'
            pooled, logit = _out(b_pooled, n * c, 'pooled').view(n, c), _out(b_logit, n, 'logit')
            dlogit, dx = _out(b_dlogit, n, 'dlogit'), _out(b_dx, n * hw * c, 'dx').view(n, hw, c)
            _assert_within(pooled, tref['pooled'], tol_p, f'{what}: pooled')
            _assert_within(logit, tref['logit'], tol_l, f'{what}: logit')
            # the forward half is the plain launch's
            _same_words(b_pooled, plain[0], f'{what}: pooled vs mcgen_dtail_loss_fused')
            _same_words(b_logit, plain[1], f'{what}: logit vs mcgen_dtail_loss_fused')
            # d loss / d logit in float64 from the logit the kernel wrote
            ref = L.lecam_d(logit[:h].float(), logit[h:].float(), loss_type, before, lam, DECAY, start)
            assert ref['active'] == (before['t'] >= start)
            assert bool(torch.isfinite(dlogit).all())
            _assert_within(dlogit, torch.cat([ref['dreal'], ref['dfake']]), torch.cat([ref['dreal_tol'], ref['dfake_tol']]),
                           f'{what}: dlogit')
            dxref, mask = R.dtail_dx(dlogit, t['x'], t['code'], t['w'], t['sigma'])
            _assert_within(dx, dxref, T._dx_tol(dxref, mask, bf16) + SUB[bf16] * mask, f'{what}: dx')
            assert bool((dx[t['x'] == 0] == 0).all())
            if not ref['active']:
                _same_words(b_dlogit, plain[2], f'{what}: inactive dlogit vs mcgen_dtail_loss_fused')
                _same_words(b_dx, plain[3], f'{what}: inactive dx vs mcgen_dtail_loss_fused')
            # the stand-alone entry on the fused launch's logits and the same state: the same derivative, bit for bit
            st_alone = _state_dev(before)
            _, a_r, a_f = _lecam_d(b_logit, b_logit[h:], h, loss_type, st_alone, lam, DECAY, start)
            assert torch.equal(torch.cat([a_r[:h], a_f[:h]]).view(torch.int32), b_dlogit[:n].view(torch.int32)), \
                f'{what}: mcgen_lecam_loss_d differs'
            # a second launch repeats the first
            again = _launch_lecam_fused(d, shape, bf16, loss_type, st, lam, start)
            for a, b, name in zip((b_pooled, b_logit, b_dlogit, b_dx), again, ('pooled', 'logit', 'dlogit', 'dx')):
                _same_words(a, b, f'{what}: second launch {name}')
        # lambda = 0 through the entry: the plain launch's bits, whatever the state
        off = _launch_lecam_fused(d, shape, bf16, loss_type, _state_dev({'a_R': 5.0, 'a_F': -5.0, 't': 9}), 0.0, 0)
        for a, b, name in zip(off, plain, ('pooled', 'logit', 'dlogit', 'dx')):
            _same_words(a, b, f'{loss_type} {shape}: lambda = 0 {name}')


# ---- 3. the paired tail-gradient launch -----------------------------------------------------------------------------------
@pytest.mark.parametrize('loss_type', LOSSES)
@pytest.mark.parametrize('n,c', [(1, 8), (3, 72), (257, 8), (1000, 72)])
def test_pair_wgrad_lecam_loss(n, c, loss_type):
    """dw1 / db1 / dw2 / db2 are mcgen_dtail_pair_wgrad's bit for bit; the loss value and the state it leaves are
    mcgen_lecam_loss_d's on the same 2N logits and state bit for bit (the same sums in the same order), and within the
    reference's bounds; inactive, the loss value is mcgen_dtail_pair_wgrad_gan_loss's."""
    lib = _lib()
    lt = L.LOSS_IDS[loss_type]
    gen = T._gen('pair-lecam', n, c)
    dlogit = torch.randn(2 * n, generator=gen)
    pooled = torch.randn(2 * n, c, generator=gen).abs() * (torch.rand(2 * n, c, generator=gen) < 0.7)
    logit = torch.cat([_logits(n, 'real'), _logits(n, 'fake').flip(0)])
    dl_d, pl_d, rt_d, lg_d = _dev(dlogit), _dev(pooled), _dev(torch.tensor([1.25])), _dev(logit)
    plain = [_nan(c), _nan(1), _nan(c), _nan(1)]
    _ok(lib.mcgen_dtail_pair_wgrad(_p(dl_d), _p(pl_d), _p(rt_d), n, c, *[_p(b) for b in plain], _stream()), 'dtail_pair_wgrad')
    lam = 0.3

    def launch(st, lam_):
        outs, loss = [_nan(c), _nan(1), _nan(c), _nan(1)], _nan(1)
        _ok(lib.mcgen_dtail_pair_wgrad_lecam_loss(_p(dl_d), _p(pl_d), _p(rt_d), _p(lg_d), n, c, *[_p(b) for b in outs], _p(loss), lt,
                                                  _p(st), lam_, DECAY, start, _stream()), 'dtail_pair_wgrad_lecam_loss')
        return outs, loss
    for before, start in TAIL_STATES + [({'a_R': 0.5, 'a_F': -0.5, 't': 0}, 3)]:
        what = f'pair lecam {loss_type} N={n} C={c} t={before["t"]} start={start}'
        st = _state_dev(before)
        outs, loss = launch(st, lam)
        for a, b, name in zip(outs, plain, ('dw1', 'db1', 'dw2', 'db2')):
            _same_words(a, b, f'{what}: {name}')
        ref = L.lecam_d(logit[:n], logit[n:], loss_type, before, lam, DECAY, start)
        got = _out(loss, 1, 'loss')
        assert bool(torch.isfinite(got).all())
        _assert_within(got, ref['loss'].view(1), ref['loss_tol'], f'{what}: loss')
        _check_state(_state_host(st), ref, before, what)
        st_alone = _state_dev(before)
        alone, _, _ = _lecam_d(lg_d, lg_d[n:], n, loss_type, st_alone, lam, DECAY, start)
        _same_words(loss, alone, f'{what}: the loss value vs mcgen_lecam_loss_d')
        assert torch.equal(st.view(torch.int32), st_alone.view(torch.int32)), f'{what}: the state vs mcgen_lecam_loss_d'
        if not ref['active']:
            old_outs, old = [_nan(c), _nan(1), _nan(c), _nan(1)], _nan(1)
            _ok(lib.mcgen_dtail_pair_wgrad_gan_loss(_p(dl_d), _p(pl_d), _p(rt_d), _p(lg_d), n, c, *[_p(b) for b in old_outs], _p(old),
                                                    lt, _stream()), 'dtail_pair_wgrad_gan_loss')
            _same_words(loss, old, f'{what}: inactive loss vs mcgen_dtail_pair_wgrad_gan_loss')
        st2 = _state_dev(before)
        outs2, loss2 = launch(st2, lam)
        _same_words(loss, loss2, f'{what}: second launch loss')
        assert torch.equal(st.view(torch.int32), st2.view(torch.int32)), f'{what}: second launch state'


# ---- 4. a sequence of updates: tail launch, then the paired launch, as a discriminator update runs them ---------------------
@pytest.mark.parametrize('loss_type', LOSSES)
def test_sequence_of_updates_follows_the_recursion(loss_type):
    """Five updates on one state, start = 2: each update's tail launch reads what the previous update's paired launch
    wrote; anchors, t and the term's switch-on follow lecam_ref update by update (each checked from the kernel's own
    previous state, so no error accumulates into the bound)."""
    shape = n, c, hw = (6, 24, 5)
    h, lam, start = n // 2, 0.5, 2
    st = _state_dev(L.fresh_state())
    for k in range(5):
        t = _spread_logits(R.tail_inputs(n, c, hw, False, True, 'seq', k))
        d = {key: _dev(v) for key, v in t.items()}
        before = {key: v for key, v in _state_host(st).items() if key in ('a_R', 'a_F', 't')}
        assert before['t'] == k
        _, b_logit, b_dlogit, _ = _launch_lecam_fused(d, shape, False, loss_type, st, lam, start)
        logit, dlogit = _out(b_logit, n, 'logit'), _out(b_dlogit, n, 'dlogit')
        ref = L.lecam_d(logit[:h].float(), logit[h:].float(), loss_type, before, lam, DECAY, start)
        assert ref['active'] == (k >= start)
        _assert_within(dlogit, torch.cat([ref['dreal'], ref['dfake']]), torch.cat([ref['dreal_tol'], ref['dfake_tol']]), f'update {k}: dlogit')
        outs, loss = [_nan(c), _nan(1), _nan(c), _nan(1)], _nan(1)
        pooled = _dev(torch.rand(n, c))
        _ok(_lib().mcgen_dtail_pair_wgrad_lecam_loss(_p(b_dlogit), _p(pooled), _p(_dev(torch.tensor([1.0]))), _p(b_logit), h, c,
                                                     *[_p(b) for b in outs], _p(loss), L.LOSS_IDS[loss_type], _p(st), lam, DECAY, start,
                                                     _stream()), 'dtail_pair_wgrad_lecam_loss')
        _assert_within(_out(loss, 1, 'loss'), ref['loss'].view(1), ref['loss_tol'], f'update {k}: loss')
        _check_state(_state_host(st), ref, before, f'update {k}')


# ---- 5. refusals on the device: an error, and nothing written ---------------------------------------------------------------
def test_refusals_leave_state_and_outputs_untouched():
    lib = _lib()
    n, c, hw = 4, 8, 2
    x, w, b, sg = _dev(torch.randn(n, hw, c)), _dev(torch.randn(c)), _dev(torch.randn(1)), _dev(torch.ones(1))
    lg = _dev(torch.randn(n))
    st = _state_dev({'a_R': 0.3, 'a_F': -0.2, 't': 5})
    keep = st.clone()

    def unchanged():
        assert torch.equal(st.view(torch.int32), keep.view(torch.int32)), 'a refused call wrote the state'
    for lam, decay, start, text in ((-0.5, 0.9, 0, 'lambda must be finite and not negative'), (float('nan'), 0.9, 0, 'lambda must be'),
                                    (0.3, 1.0, 0, 'decay in [0, 1)'), (0.3, -0.1, 0, 'decay in [0, 1)'),
                                    (0.3, 0.9, -1, 'start must not be negative')):
        loss, dr, df = _nan(1), _nan(2), _nan(2)
        _refused(lib.mcgen_lecam_loss_d(_p(lg), _p(lg[2:]), 2, 0, _p(st), lam, decay, start, _p(loss), _p(dr), _p(df), _stream()),
                 'lecam_loss_d: ' + text, loss, dr, df)
        unchanged()
        outs, lo = [_nan(c), _nan(1), _nan(c), _nan(1)], _nan(1)
        _refused(lib.mcgen_dtail_pair_wgrad_lecam_loss(_p(lg), _p(x), _p(sg), _p(lg), 2, c, *[_p(o) for o in outs], _p(lo), 1, _p(st),
                                                       lam, decay, start, _stream()), 'dtail_pair_wgrad_lecam_loss: ' + text, lo, *outs)
        unchanged()
        if 'decay' not in text:
            outs = [_nan(n * c), _nan(n), _nan(n), _nan(n * hw * c)]
            _refused(lib.mcgen_dtail_lecam_fused(_p(x), _dtc(False), None, _p(w), _p(b), _p(sg), *[_p(o) for o in outs], n, hw, c, 1,
                                                 _p(st), lam, start, _stream()), 'dtail_lecam_fused: ' + text, *outs)
            unchanged()
    loss, dr, df = _nan(1), _nan(2), _nan(2)
    _refused(lib.mcgen_lecam_loss_d(_p(lg), _p(lg[2:]), 2, 0, None, 0.3, 0.9, 0, _p(loss), _p(dr), _p(df), _stream()),
             'lecam_loss_d: null state', loss, dr, df)
    outs = [_nan(n * c), _nan(n), _nan(n), _nan(n * hw * c)]
    _refused(lib.mcgen_dtail_lecam_fused(_p(x), _dtc(False), None, _p(w), _p(b), _p(sg), *[_p(o) for o in outs], 3, hw, c, 1,
                                         _p(st), 0.3, 0, _stream()), 'dtail_lecam_fused: a paired batch (N even and positive)', *outs)
    unchanged()
