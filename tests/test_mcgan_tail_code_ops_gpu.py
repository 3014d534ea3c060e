"""The kernels of csrc/small_ops.hip that test_mcgan_small_ops_gpu.py leaves out, one at a time: the discriminator tail
(forward, input gradient, weight gradients, the fused tail + hinge launch), the hinge losses, tanh backward, the
MultimodalController codes (product, batched product, label gather, apply), the compaction maps and their affine rows,
the one-hot indicator and the layout kernels (NCHW <-> NHWC, 2x2 sum pooling).

Every reference is float64 on the CPU (tests/small_ops_ref.py, checked against torch in test_small_ops_ref_cpu.py),
computed from exactly the values the kernel read: bf16 activations as their exact values, fp32 scalars as fp32 values.
No bound is measured on the code under test; each follows from the output type, the number of operations and the
magnitudes of the terms:

- u = 2^-24 is the fp32 unit roundoff.  A chain of n fp32 additions or fmas, in any order and any grouping, errs by at
  most n u (sum of the magnitudes of its terms); an addition of an exact zero is exact, so idle lanes and empty sample
  quarters cost nothing.  A bound is doubled where a device division (within 2u) or second-order terms enter.  A bf16
  store adds 2^-8 relative to the stored value (half a bf16 ulp).
- tail forward.  pooled[n][c] = code sum_hw relu(x): HW - 1 additions and one product: HW u sum |terms|, and exactly 0
  where every term is 0 (x <= 0 of either sign, or code 0).  logit[n] = sum_c pooled w / sigma + b: the pooled bound
  carried through |w / sigma|, plus C fmas, the bias and the division of w by sigma: (C + 2) u sum |terms|, doubled.
- tail input gradient.  dx = dlogit w (1 / sigma) code where x > 0, else 0: the mask is exact (tolerance 0 where
  x <= 0, and a value within 5u of a non-zero reference is non-zero); three products and one reciprocal: 5u relative;
  bf16 adds 2^-8.
- tail weight gradients.  dw[c] = sum_n dlogit pooled is a dot product of length N: N u sum |terms|; with `accumulate`
  one more addition: (N + 1) u (|dw before| + sum |terms|); dw2's division by `ratio`: (N + 1) u sum |terms| / ratio,
  doubled.  db = sum_n dlogit: N u sum |dlogit|, (N + 1) u (|db before| + sum |dlogit|) with `accumulate`.
- hinge losses.  1 - real and 1 + fake decide the gradient: fp32 subtraction is exact near 1 and never changes the sign
  of an inexact difference, so d loss / d logit EQUALS -+fl(1 / N) or 0 as the float64 reference decides, 0 at the
  hinge point itself (torch.relu's gradient at 0).  The loss: per term one subtraction, N - 1 additions, 1 / N, one
  product and the final addition -- (N + 2) u sum |terms|, doubled; the same for mcgen_dtail_pair_wgrad_loss's block and
  for hinge_g (no subtraction, no final addition).
- the fused tail: the forward bounds above; d loss / d logit equals the reference's decision.  That needs every
  reference logit further than 4 logit bounds from its hinge point: an input condition, asserted (never allowed for)
  here and in test_small_ops_ref_cpu.py.  In the dyadic cases every partial sum is an fp32 number in any order
  (small_ops_ref.assert_exact, from the reference alone): logit, pooled, dlogit and dx compare for equality.
- tanh backward.  a = fl(y y), b = fl(1 - a), dx = fl(dy b): |dy| (|1 - y^2| ((1 + u)^2 - 1) + y^2 u (1 + u)^2), the
  three roundings written out (an fma in place of the first two only errs less); bf16 adds 2^-8 (|ref| + that bound).
- codes.  A one-hot row times the codebook has one non-zero term, 1.0 * codebook[label][c]: equality.  A row scaled by
  `scale` is one fp32 product; the float64 product of two fp32 numbers is exact, so rounding it once to fp32 is the
  correctly rounded answer: equality.  A soft indicator: M fmas, M u sum |terms|, (M + 1) u |scale| sum |terms| where
  the row is scaled too.  mc_apply is one product (fp32: equality with the rounded float64 product; bf16: equality with
  its round-to-nearest-even).  mc_affine's entries are single products: equality.  Maps and indicators are integers.
- layout.  NCHW <-> NHWC moves values: equality in fp32, round-to-nearest-even (small_ops_ref.round_bf16) in bf16.
  pool2_sum is (a + b) + (c + d): 2u sum |terms|; bf16 adds 2^-8 (|ref| + that bound); on multiples of 1/4 in [-4, 4]
  every sum is a bf16 number: equality.

Buffers a kernel writes only in part start as NaN (int16 maps: a sentinel word) and must keep it where the kernel must
not write; every output is followed by such a gap.  After every launch _sync() waits for the device and ends the whole
session on a device error: nothing more is launched on a faulted GPU."""

import pytest
import torch
import torch.nn.functional as F

import small_ops_ref as R

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U16 = 2.0 ** -8
NAN = float('nan')
GAP = 8
F64 = torch.float64
SENT16 = 0x5A5A
# thresholds that live only in csrc/small_ops.hip
GRID_CAP = 4096 * 256       # grid_for's default: 4096 blocks of 256 threads, then the loop wraps
CODE_GRID = 128 * 256       # mc_code_batch_kernel: 128 blocks per module
GATHER_GRID = 8 * 256 * 4   # mc_gather_batch_kernel: 8 blocks per module, four floats per thread
ONEHOT_GRID = 256 * 256     # onehot_rep_kernel: 256 blocks at most


def _ops():
    from mcgen_amd import ops
    return ops


def _L():
    from mcgen_amd import _lib
    return _lib


def _lib():
    return _L().load()


_KEEP = []        # device copies made for a launch: alive until the launch has finished


def _sync():
    """Wait for the launch; a device-side fault ends the whole session -- nothing more is launched on a faulted GPU."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault, stopping the session: {e}', returncode=3)
    del _KEEP[:]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(t):
    """A contiguous device copy that stays alive until the next _sync()."""
    if t is None:
        return None
    _KEEP.append(t.contiguous().cuda())
    return _KEEP[-1]


def _dt(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _dtc(bf16):
    return _L().BF16 if bf16 else _L().F32


def _nan(n, dtype=torch.float32):
    """n elements and a gap, all NaN, on the device."""
    return torch.full((n + GAP,), NAN, dtype=dtype, device='cuda')


def _ok(rc, what):
    assert rc == 0, f'{what}: {_lib().mcgen_last_error().decode()}'
    _sync()


def _refused(rc, text, *sentinels):
    """The call returned an error with `text` in it, and wrote nothing: every sentinel buffer is still all NaN."""
    _sync()
    assert rc != 0, f'accepted, expected a refusal with "{text}"'
    msg = _lib().mcgen_last_error().decode()
    assert text in msg, f'refused with "{msg}", expected "{text}"'
    for s in sentinels:
        assert bool(torch.isnan(s.float()).all()), 'a refused call wrote into its output'


def _out(buf, n, what):
    """The first n elements of a NaN-gapped buffer as float64 on the CPU; the gap must still be NaN."""
    b = buf.detach().float().cpu()
    assert bool(torch.isnan(b[n:]).all()), f'{what}: wrote past its {n} elements'
    return b[:n].double()


def _assert_within(got, ref, tol, what):
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        tol = tol.expand_as(ref) if torch.is_tensor(tol) else torch.full_like(ref, tol)
        raise AssertionError(f'{what}: {int(bad.sum())} of {err.numel()} outside the bound; first at flat index {i}: '
                             f'got {float(got.flatten()[i])}, ref {float(ref.flatten()[i])}, tol {float(tol.flatten()[i])}')


def _assert_equal(got, ref, what):
    """Equality of values (-0.0 == 0.0); NaN anywhere fails."""
    got = got.detach().double().cpu().reshape(ref.shape)
    bad = ~(got == ref.double())
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} differ; first at flat index {i}: '
                             f'got {float(got.flatten()[i])}, ref {float(ref.flatten()[i])}')


def _gen(*key):
    return torch.Generator().manual_seed(R.seed_of(*key))


# ---- 1. discriminator tail ----------------------------------------------------------------------------------------------
def _tail_ref(t):
    return R.dtail(t['x'], t['code'], t['w'], t['b'], t['sigma'])


def _tail_dev(t, bf16):
    return {k: (_dev(v.to(_dt(bf16))) if k == 'x' else _dev(v)) for k, v in t.items()}


def _launch_fwd(t, bf16):
    """mcgen_dtail_fwd into NaN-gapped buffers -> (pooled [N, C], logit [N]) as float64."""
    n, hw, c = t['x'].shape
    d = _tail_dev(t, bf16)
    pooled, logit = _nan(n * c), _nan(n)
    _ok(_lib().mcgen_dtail_fwd(_p(d['x']), _dtc(bf16), _p(d['code']), _p(d['w']), _p(d['b']), _p(d['sigma']), _p(pooled), _p(logit),
                               n, hw, c, _stream()), 'dtail_fwd')
    return _out(pooled, n * c, 'pooled').view(n, c), _out(logit, n, 'logit')


def _launch_fused(t, bf16, mode):
    """mcgen_dtail_hinge_fused into NaN-gapped buffers -> (pooled, logit, dlogit, dx [N, HW, C]) as float64."""
    n, hw, c = t['x'].shape
    d = _tail_dev(t, bf16)
    pooled, logit, dlogit, dx = _nan(n * c), _nan(n), _nan(n), _nan(n * hw * c, _dt(bf16))
    _ok(_lib().mcgen_dtail_hinge_fused(_p(d['x']), _dtc(bf16), _p(d['code']), _p(d['w']), _p(d['b']), _p(d['sigma']), _p(pooled),
                                       _p(logit), _p(dlogit), _p(dx), n, hw, c, {'d_pair': 0, 'g': 1}[mode], _stream()), 'dtail_hinge_fused')
    return (_out(pooled, n * c, 'pooled').view(n, c), _out(logit, n, 'logit'), _out(dlogit, n, 'dlogit'),
            _out(dx, n * hw * c, 'dx').view(n, hw, c))


def _launch_bwd(t, bf16, dlogit, pooled=None, dw=None, db=None, accumulate=0):
    """mcgen_dtail_bwd -> dx [N, HW, C] as float64 (dw / db, NaN-gapped device buffers, are updated in place)."""
    n, hw, c = t['x'].shape
    d = _tail_dev(t, bf16)
    dx = _nan(n * hw * c, _dt(bf16))
    pooled = torch.zeros(n, c, device='cuda') if pooled is None else pooled
    _ok(_lib().mcgen_dtail_bwd(_p(_dev(dlogit)), _p(d['x']), _dtc(bf16), _p(d['code']), _p(d['w']), _p(d['sigma']), _p(pooled), _p(dx),
                               _p(dw), _p(db), n, hw, c, accumulate, _stream()), 'dtail_bwd')
    return _out(dx, n * hw * c, 'dx').view(n, hw, c)


def _check_forward(t, ref, pooled, logit, what):
    tol_p, tol_l = R.tail_bounds(t, ref)
    _assert_within(pooled, ref['pooled'], tol_p, f'{what}: pooled')
    _assert_within(logit, ref['logit'], tol_l, f'{what}: logit')


def _dx_tol(dxref, mask, bf16):
    """5u relative where x > 0 (bf16: + 2^-8), 0 where the mask is closed."""
    return dxref.abs() * (5 * U32 + (U16 if bf16 else 0.0)) * mask


def _decision(ref, mode):
    """d loss / d logit as the reference logits decide it, in fp32 values: the kernel must EQUAL this."""
    n = ref['logit'].numel()
    if mode == 'g':
        return R.hinge_g(ref['logit'])[1].sign() * R.f32(1.0 / n)
    h = n // 2
    _, dr, df, _ = R.hinge_d(ref['logit'][:h], ref['logit'][h:])
    return torch.cat([dr, df]).sign() * R.f32(1.0 / h)


def _check_fused(t, bf16, mode, what, exact=False):
    ref = _tail_ref(t)
    tol_l = R.tail_bounds(t, ref)[1]
    assert exact or not bool(R.undecided(ref, tol_l, mode).any()), f'{what}: an undecided sample: a broken case'
    pooled, logit, dlogit, dx = _launch_fused(t, bf16, mode)
    dl = _decision(ref, mode)
    dxref, mask = R.dtail_dx(dl, t['x'], t['code'], t['w'], t['sigma'])
    if exact:
        _assert_equal(pooled, ref['pooled'], f'{what}: pooled')
        _assert_equal(logit, ref['logit'], f'{what}: logit')
        _assert_equal(dlogit, dl, f'{what}: dlogit')
        _assert_equal(dx, R.round_bf16(dxref) if bf16 else dxref, f'{what}: dx')
    else:
        _check_forward(t, ref, pooled, logit, what)
        _assert_equal(dlogit, dl, f'{what}: dlogit')
        _assert_within(dx, dxref, _dx_tol(dxref, mask, bf16), f'{what}: dx')
    return ref, dl


FWD_CASES = [(s, 'fwd') for s in R.TAIL_SHAPES + R.TAIL_SCALAR_SHAPES] + [(s, 'fused') for s in R.TAIL_SHAPES]


@pytest.mark.parametrize('with_code', [True, False])
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('shape,kernel', FWD_CASES)
def test_tail_forward(shape, kernel, bf16, with_code):
    """mcgen_dtail_fwd (the vector kernel with 256 / (C / 8) pixel lanes, the scalar kernel where C % 8 != 0 or C > 2048)
    and the forward half of mcgen_dtail_hinge_fused (mode g takes any N, odd ones too; its dlogit = -fl(1 / N) and dx are
    checked with it).  About 1 in 16 entries of x is 0.0 and 1 in 16 is -0.0, the last channel holds nothing else: they
    pool as exactly zero."""
    t = R.tail_inputs(*shape, bf16, with_code)
    what = f'{kernel} {shape} bf16={bf16} code={with_code}'
    if kernel == 'fused':
        _check_fused(t, bf16, 'g', what)
        return
    ref = _tail_ref(t)
    pooled, logit = _launch_fwd(t, bf16)
    _check_forward(t, ref, pooled, logit, what)
    assert bool((pooled[:, -1] == 0).all())


@pytest.mark.parametrize('with_code', [True, False])
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('shape', R.TAIL_SHAPES + R.TAIL_SCALAR_SHAPES + [(130, 128, 64)])
def test_tail_input_gradient(shape, bf16, with_code):
    """mcgen_dtail_bwd's dx for a random dlogit (no dw / db: NULL is accepted); (130, 128, 64) has 1 064 960 elements
    against 4096 x 256 threads, so dtail_bwd_dx's loop wraps."""
    n, c, hw = shape
    assert (n * c * hw > GRID_CAP) == (shape == (130, 128, 64))
    t = R.tail_inputs(*shape, bf16, with_code)
    dlogit = torch.randn(n, generator=_gen('dx', shape)) / n
    dx = _launch_bwd(t, bf16, dlogit)
    dxref, mask = R.dtail_dx(dlogit, t['x'], t['code'], t['w'], t['sigma'])
    _assert_within(dx, dxref, _dx_tol(dxref, mask, bf16), f'dx {shape}')
    assert bool((dx[t['x'] == 0] == 0).all())


@pytest.mark.parametrize('c', [8, 40, 64, 72, 512])
@pytest.mark.parametrize('n', [1, 2, 3, 5, 64, 257])
def test_tail_weight_gradients(n, c):
    """dw / db of mcgen_dtail_bwd (N samples; accumulate 0 over a NaN start, which it must overwrite, and accumulate 1 on a
    random start) and of mcgen_dtail_pair_wgrad / mcgen_dtail_pair_wgrad_loss (2N samples, ratio 1.25).  N = 1, 2, 3 leave
    sample quarters empty, 5 and 257 are no multiple of 4; C = 72, 512 take more than one 64-channel block.  The loss block
    leaves dw / db bit for bit what the form without a loss writes."""
    lib = _lib()
    gen = _gen('wgrad', n, c)
    dlogit = torch.randn(2 * n, generator=gen)
    pooled = torch.randn(2 * n, c, generator=gen).abs() * (torch.rand(2 * n, c, generator=gen) < 0.7)
    logit = torch.randn(2 * n, generator=gen) * 2
    ratio = torch.tensor([1.25])
    t = {'x': torch.randn(n, 1, c, generator=gen), 'code': None, 'w': torch.randn(c, generator=gen), 'b': None,
         'sigma': torch.tensor([1.7])}
    # mcgen_dtail_bwd over the first N samples
    dw, db, dwa, dba = R.dtail_wgrad(dlogit[:n], pooled[:n])
    for start in (None, 'random'):
        gdw, gdb = _nan(c), _nan(1)
        dw0, db0 = torch.zeros(c, dtype=F64), torch.zeros((), dtype=F64)
        if start:
            dw0, db0 = torch.randn(c, generator=gen), torch.randn((), generator=gen)
            gdw[:c], gdb[:1] = dw0.cuda(), db0.cuda()
            dw0, db0 = dw0.double(), db0.double()
        _launch_bwd(t, False, dlogit[:n], _dev(pooled[:n]), gdw, gdb, accumulate=1 if start else 0)
        k = n + 1 if start else n
        _assert_within(_out(gdw, c, 'dw'), dw0 + dw, k * U32 * (dw0.abs() + dwa), f'dtail_bwd dw, start {start}')
        _assert_within(_out(gdb, 1, 'db'), (db0 + db).view(1), k * U32 * (db0.abs() + dba), f'dtail_bwd db, start {start}')
    # the paired forms
    (dw1, db1, dw1a, db1a), (dw2, db2, dw2a, db2a) = R.dtail_pair_wgrad(dlogit, pooled, 1.25)
    dl_d, pl_d, rt_d, lg_d = _dev(dlogit), _dev(pooled), _dev(ratio), _dev(logit)
    plain = [_nan(c), _nan(1), _nan(c), _nan(1)]
    _ok(lib.mcgen_dtail_pair_wgrad(_p(dl_d), _p(pl_d), _p(rt_d), n, c, *[_p(b) for b in plain], _stream()), 'dtail_pair_wgrad')
    _assert_within(_out(plain[0], c, 'dw1'), dw1, n * U32 * dw1a, 'pair dw1')
    _assert_within(_out(plain[1], 1, 'db1'), db1.view(1), n * U32 * db1a, 'pair db1')
    _assert_within(_out(plain[2], c, 'dw2'), dw2, 2 * (n + 1) * U32 * dw2a, 'pair dw2 (divided by ratio)')
    _assert_within(_out(plain[3], 1, 'db2'), db2.view(1), n * U32 * db2a, 'pair db2')
    withl = [_nan(c), _nan(1), _nan(c), _nan(1)]
    loss = _nan(1)
    _ok(lib.mcgen_dtail_pair_wgrad_loss(_p(dl_d), _p(pl_d), _p(rt_d), _p(lg_d), n, c, *[_p(b) for b in withl], _p(loss), _stream()),
        'dtail_pair_wgrad_loss')
    for a, b in zip(plain, withl):
        assert torch.equal(a[:-GAP], b[:-GAP]) and bool(torch.isnan(b[-GAP:]).all()), 'the loss block changed dw / db'
    lref, _, _, labs = R.hinge_d(logit[:n], logit[n:])
    _assert_within(_out(loss, 1, 'loss'), lref.view(1), 2 * (n + 2) * U32 * labs, 'pair loss')


# ---- 2. hinge decisions -------------------------------------------------------------------------------------------------
EDGE_LOGITS = [1.0, -1.0, 1 + 2.0 ** -23, 1 - 2.0 ** -23, -1 + 2.0 ** -23, -1 - 2.0 ** -23]


def _hinge_vectors(n):
    """(real, fake) pairs of N logits that hold every edge logit (N = 1: one pair per edge)."""
    gen = _gen('hinge', n)
    if n < len(EDGE_LOGITS):
        return [(torch.tensor([e]), torch.tensor([-e])) for e in EDGE_LOGITS] + [(torch.tensor([e]), torch.tensor([e])) for e in EDGE_LOGITS]
    real, fake = torch.randn(n, generator=gen) * 2, torch.randn(n, generator=gen) * 2
    edge = torch.tensor(EDGE_LOGITS)
    real[:6], fake[:6] = edge, edge.flip(0)
    real[-6:], fake[-6:] = edge.flip(0), edge         # the last entries too: past the first block of 256 where N > 256
    return [(real, fake)]


@pytest.mark.parametrize('n', [1, 6, 256, 257, 1000])
def test_hinge_losses(n):
    """mcgen_hinge_d and mcgen_hinge_g: logits exactly 1, -1, 1 +- 2^-23, -1 +- 2^-23 among random ones; the gradients
    equal -+fl(1 / N) or 0 as the reference decides (0 at the hinge point), the losses within (N + 2) u sum |terms|, doubled."""
    lib = _lib()
    assert all(float(torch.tensor(e, dtype=torch.float32)) == e for e in EDGE_LOGITS)
    inv = R.f32(1.0 / n)
    for real, fake in _hinge_vectors(n):
        loss, dr, df = _nan(1), _nan(n), _nan(n)
        _ok(lib.mcgen_hinge_d(_p(_dev(real)), _p(_dev(fake)), n, _p(loss), _p(dr), _p(df), _stream()), 'hinge_d')
        lref, drr, dfr, labs = R.hinge_d(real, fake)
        assert bool((drr[real.double() == 1] == 0).all()) and bool((dfr[fake.double() == -1] == 0).all())
        _assert_equal(_out(dr, n, 'dreal'), drr.sign() * inv, f'hinge_d dreal, N = {n}')
        _assert_equal(_out(df, n, 'dfake'), dfr.sign() * inv, f'hinge_d dfake, N = {n}')
        _assert_within(_out(loss, 1, 'loss'), lref.view(1), 2 * (n + 2) * U32 * labs, f'hinge_d loss, N = {n}')
        loss, df = _nan(1), _nan(n)
        _ok(lib.mcgen_hinge_g(_p(_dev(fake)), n, _p(loss), _p(df), _stream()), 'hinge_g')
        lref, dfr, labs = R.hinge_g(fake)
        _assert_equal(_out(df, n, 'dfake'), dfr.sign() * inv, f'hinge_g dfake, N = {n}')
        _assert_within(_out(loss, 1, 'loss'), lref.view(1), 2 * (n + 2) * U32 * labs, f'hinge_g loss, N = {n}')


@pytest.mark.parametrize('mode', ['d_pair', 'g'])
@pytest.mark.parametrize('with_code', [True, False])
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('shape', R.TAIL_EXACT_SHAPES)
def test_fused_tail_exact(shape, bf16, with_code, mode):
    """Dyadic inputs on which every fp32 partial sum is exact in any order (asserted from the reference): samples 0 and h
    have logit exactly +1, samples 1 and h + 1 exactly -1, samples 2 and h + 2 exactly 0 (h = N / 2 = 4), so in mode
    d_pair dlogit must be 0, -1/4, -1/4 in the first half and +1/4, 0, +1/4 in the second.  pooled, logit, dlogit and dx
    (products of few-bit dyadic numbers) compare for equality, from mcgen_dtail_hinge_fused and from mcgen_dtail_fwd."""
    t = R.tail_exact_inputs(*shape, with_code=with_code)
    R.assert_exact(R.tail_exact_bits(t), f'tail {shape}')
    assert torch.equal(t['x'].bfloat16().float(), t['x'])
    ref, dl = _check_fused(t, bf16, mode, f'exact {shape} bf16={bf16} code={with_code} {mode}', exact=True)
    h = shape[0] // 2
    assert ref['logit'][[0, 1, 2, h, h + 1, h + 2]].tolist() == [1.0, -1.0, 0.0, 1.0, -1.0, 0.0]
    if mode == 'd_pair':
        assert dl[[0, 1, 2, h, h + 1, h + 2]].tolist() == [0.0, -0.25, -0.25, 0.25, 0.0, 0.25]
    pooled, logit = _launch_fwd(t, bf16)
    _assert_equal(pooled, ref['pooled'], 'dtail_fwd pooled')
    _assert_equal(logit, ref['logit'], 'dtail_fwd logit')


@pytest.mark.parametrize('with_code', [True, False])
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('shape', R.FUSED_RANDOM)
def test_fused_tail_hinge_decisions(shape, bf16, with_code):
    """mcgen_dtail_hinge_fused in mode d_pair on random inputs: no reference logit within 4 logit bounds of its hinge
    point (asserted: the seeds are chosen so), hence dlogit equals the reference's decision -- which half a sample is in,
    which side of the hinge its logit is on; pooled, logit and dx to the tail bounds.  (2, 40, 5) is one real and one
    generated sample."""
    t = R.fused_inputs(*shape, bf16, with_code)
    ref = _tail_ref(t)
    assert not bool(R.undecided(ref, R.tail_bounds(t, ref)[1], 'd_pair').any()), 'an undecided sample: a broken case'
    _, dl = _check_fused(t, bf16, 'd_pair', f'fused {shape} bf16={bf16} code={with_code}')
    h = shape[0] // 2
    assert bool((dl[:h] <= 0).all()) and bool((dl[h:] >= 0).all())


@pytest.mark.parametrize('n,c,mode,text', [(4, 12, 1, 'C must be a multiple of 8, at most 2048'),
                                          (4, 2056, 1, 'C must be a multiple of 8, at most 2048'),
                                          (5, 8, 0, 'mode 0 (hinge_d over a paired batch, N even) or 1 (hinge_g)')])
def test_fused_tail_refusals(n, c, mode, text):
    hw = 2
    x, w, b, sigma = torch.ones(n, hw, c, device='cuda'), torch.ones(c, device='cuda'), torch.ones(1, device='cuda'), torch.ones(1, device='cuda')
    outs = [_nan(n * c), _nan(n), _nan(n), _nan(n * hw * c)]
    rc = _lib().mcgen_dtail_hinge_fused(_p(x), _L().F32, None, _p(w), _p(b), _p(sigma), *[_p(o) for o in outs], n, hw, c, mode, _stream())
    _refused(rc, 'dtail_hinge_fused: ' + text, *outs)


# ---- 3. tanh backward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n', [1, 7, GRID_CAP, GRID_CAP + 1 + 255])
def test_tanh_bwd(n, bf16):
    """dx = dy (1 - y^2); y holds exact 1, -1 and 0 (n = 1: one launch each); 4096 x 256 elements fill the grid exactly,
    256 more take a second trip of the loop."""
    gen = _gen('tanh', n, bf16)
    starts = [[1.0], [-1.0], [0.0]] if n == 1 else [[1.0, -1.0, 0.0]]
    for head in starts:
        y, dy = torch.tanh(torch.randn(n, generator=gen) * 2), torch.randn(n, generator=gen)
        y[:len(head)] = torch.tensor(head)
        y[-len(head):] = torch.tensor(head)
        y, dy = y.to(_dt(bf16)), dy.to(_dt(bf16))
        dx = _nan(n, _dt(bf16))
        _ok(_lib().mcgen_tanh_bwd(_p(_dev(dy)), _p(_dev(y)), _p(dx), _dtc(bf16), n, _stream()), 'tanh_bwd')
        y64, dy64 = y.double(), dy.double()
        ref = R.tanh_bwd(dy64, y64)
        tol = dy64.abs() * ((1 - y64 ** 2).abs() * ((1 + U32) ** 2 - 1) + y64 ** 2 * U32 * (1 + U32) ** 2)
        if bf16:
            tol = tol + U16 * (ref.abs() + tol)
        got = _out(dx, n, 'dx')
        _assert_within(got, ref, tol, f'tanh_bwd n = {n}')
        assert bool((got[y64.abs() == 1] == 0).all()) and bool((got[y64 == 0] == dy64[y64 == 0]).all())


# ---- 4. codes -----------------------------------------------------------------------------------------------------------
def _codebook(gen, m, c):
    """Non-binary floats, about half of them zero, every row different: a wrong row cannot pass."""
    return (torch.rand(m, c, generator=gen) < 0.5).float() * (0.5 + torch.rand(m, c, generator=gen)) + torch.arange(m).view(m, 1) * 2.0 ** -12


def _soft(gen, n, m):
    """A soft indicator with negative entries and exact zeros."""
    s = torch.rand(n, m, generator=gen) - 0.3
    s[torch.rand(n, m, generator=gen) < 0.25] = 0.0
    return s


def _code_table(cbs, n):
    """A descriptor table over device codebooks with a NaN gap after every module's [n, C] block -> (table, offsets, total)."""
    arr = (_L().Code * len(cbs))()
    off, offs = 0, []
    for d, (cb, sidx) in zip(arr, cbs):
        d.codebook, d.out_off, d.M, d.C, d.scale_idx = cb.data_ptr(), off, cb.shape[0], cb.shape[1], sidx
        offs.append(off)
        off += n * cb.shape[1] + GAP
    return _ops()._struct_table(arr, 'cuda'), offs, off


def _check_codes(buf, offs, total, cbs, n, want, tols, what):
    flat = buf.detach().cpu()
    keep = torch.ones(total, dtype=torch.bool)
    for j, (off, (cb, _)) in enumerate(zip(offs, cbs)):
        c = cb.shape[1]
        keep[off:off + n * c] = False
        got = flat[off:off + n * c].view(n, c)
        if tols is None:
            _assert_equal(got, want[j], f'{what}: module {j} (C = {c})')
        else:
            _assert_within(got, want[j], tols[j], f'{what}: module {j} (C = {c})')
    assert bool(torch.isnan(flat[keep]).all()), f'{what}: wrote into a gap'


CODE_CS = (8, 36, 512)
CODE_N = 66


@pytest.mark.parametrize('m', [10, 32, 33, 100, 1623])
def test_code_products_one_hot(m):
    """mcgen_mc_code and mcgen_mc_code_batch (three modules of C = 8, 36, 512 in one launch, a NaN gap after each, and
    through ops.CodeBatch.run) on one-hot indicators: code == codebook[label]; with `scale` and n_half = 23 the rows from 23
    on equal fl(code scale) and the rows below are untouched; the module with scale_idx -1 is not scaled.  66 x 512 outputs
    are more than the 128 x 256 threads of a module's grid row: the loop wraps.  M = 32 / 33 are the two sides of
    mc_code_batch's unrolled / skipping branch."""
    ops, lib = _ops(), _lib()
    n, n_half = CODE_N, 23
    assert n * CODE_CS[-1] > CODE_GRID
    gen = _gen('code', m)
    label = torch.randint(0, m, (n,), generator=gen)
    label[0], label[1] = 0, m - 1
    ind = _dev(F.one_hot(label, m).float())
    cbs_cpu = [_codebook(gen, m, c) for c in CODE_CS]
    cbs = [(_dev(cb), sidx) for cb, sidx in zip(cbs_cpu, (1, -1, 0))]
    scale = torch.rand(2, generator=gen) + 0.5
    for cb, (cbd, _) in zip(cbs_cpu, cbs):
        c = cb.shape[1]
        code = _nan(n * c)
        _ok(lib.mcgen_mc_code(_p(ind), _p(cbd), _p(code), n, m, c, _stream()), 'mc_code')
        _assert_equal(_out(code, n * c, 'mc_code').view(n, c), R.mc_code(F.one_hot(label, m).float(), cb), f'mc_code M = {m}, C = {c}')
        assert torch.equal(_out(code, n * c, 'mc_code').view(n, c), cb[label].double())
    table, offs, total = _code_table(cbs, n)
    for sc in (None, scale):
        buf = torch.full((total,), NAN, device='cuda')
        _ok(lib.mcgen_mc_code_batch(_p(ind), _p(table), len(cbs), _p(buf), n, _p(_dev(sc)), n_half, _stream()), 'mc_code_batch')
        want = []
        for cb, (_, sidx) in zip(cbs_cpu, cbs):
            s = None if sc is None or sidx < 0 else float(sc[sidx])
            w = R.mc_code(F.one_hot(label, m).float(), cb, n_half, s)
            assert torch.equal(w[:n_half], cb[label][:n_half].double())
            want.append(w.float().double())                  # the exact product rounded once
        _check_codes(buf, offs, total, cbs, n, want, None, f'mc_code_batch M = {m}, scale {sc is not None}')

    class MC:
        pass
    mcs = []
    for cbd, _ in cbs:
        mc = MC(); mc.codebook = cbd; mcs.append(mc)
    outs = ops.CodeBatch(mcs, [1, -1, 0]).run(ind, _dev(scale), n_half)
    _sync()
    for o, w in zip(outs, want):
        _assert_equal(o, w, 'CodeBatch.run')


@pytest.mark.parametrize('m', [32, 33])
def test_code_products_soft_indicator(m):
    """A soft indicator (negative entries, exact zeros) through mcgen_mc_code and both branches of mc_code_batch_kernel
    (M <= 32: every term; M > 32: zero entries skipped): M fmas, M u sum |terms|; the scaled rows one product more."""
    lib = _lib()
    n, n_half = CODE_N, 23
    gen = _gen('soft', m)
    soft = _soft(gen, n, m)
    cbs_cpu = [_codebook(gen, m, c) - 0.25 for c in CODE_CS]
    cbs = [(_dev(cb), sidx) for cb, sidx in zip(cbs_cpu, (1, -1, 0))]
    scale = torch.rand(2, generator=gen) + 0.5
    table, offs, total = _code_table(cbs, n)
    buf = torch.full((total,), NAN, device='cuda')
    _ok(lib.mcgen_mc_code_batch(_p(_dev(soft)), _p(table), len(cbs), _p(buf), n, _p(_dev(scale)), n_half, _stream()), 'mc_code_batch')
    want, tols = [], []
    for cb, (cbd, sidx) in zip(cbs_cpu, cbs):
        c = cb.shape[1]
        s = 1.0 if sidx < 0 else float(scale[sidx])
        want.append(R.mc_code(soft, cb, n_half, s))
        tol = m * U32 * (soft.double().abs() @ cb.double().abs())
        if sidx >= 0:
            tol[n_half:] *= (m + 1) / m * abs(s)
        tols.append(tol)
        code = _nan(n * c)
        _ok(lib.mcgen_mc_code(_p(_dev(soft)), _p(cbd), _p(code), n, m, c, _stream()), 'mc_code')
        _assert_within(_out(code, n * c, 'mc_code').view(n, c), R.mc_code(soft, cb), m * U32 * (soft.double().abs() @ cb.double().abs()),
                       f'mc_code soft M = {m}, C = {c}')
    _check_codes(buf, offs, total, cbs, n, want, tols, f'mc_code_batch soft M = {m}')


@pytest.mark.parametrize('reps', [1, 2, 5])
@pytest.mark.parametrize('m', [10, 33, 1623])
def test_code_gather_by_label(m, reps):
    """mcgen_mc_gather_batch (raw, NaN gaps, and through ops.CodeBatch.run_labels): the label vector repeats `reps` times;
    labels -1 and M are clamped to rows 0 and M - 1 as the header says; 24 reps x 512 floats are more than the 8 x 256
    threads x 4 floats of a module's grid row; scale / n_half as in the product."""
    ops, lib = _ops(), _lib()
    nl = 24
    n, n_half = nl * reps, nl * reps // 2 + 1
    assert n * 512 > GATHER_GRID
    gen = _gen('gather', m, reps)
    label = torch.randint(0, m, (nl,), generator=gen)
    label[3], label[4], label[5], label[6] = -1, m, 0, m - 1
    clamped = label.clamp(0, m - 1).repeat(reps)
    cbs_cpu = [_codebook(gen, m, c) for c in CODE_CS]
    cbs = [(_dev(cb), sidx) for cb, sidx in zip(cbs_cpu, (1, -1, 0))]
    scale = torch.rand(2, generator=gen) + 0.5
    table, offs, total = _code_table(cbs, n)
    for sc in (None, scale):
        buf = torch.full((total,), NAN, device='cuda')
        _ok(lib.mcgen_mc_gather_batch(_p(_dev(label)), nl, _p(table), len(cbs), _p(buf), n, _p(_dev(sc)), n_half, _stream()), 'mc_gather_batch')
        want = []
        for cb, (_, sidx) in zip(cbs_cpu, cbs):
            s = None if sc is None or sidx < 0 else float(sc[sidx])
            want.append(R.mc_code(F.one_hot(clamped, m).float(), cb, n_half, s).float().double())
        _check_codes(buf, offs, total, cbs, n, want, None, f'mc_gather_batch M = {m}, reps {reps}, scale {sc is not None}')

    class MC:
        pass
    mcs = []
    for cbd, _ in cbs:
        mc = MC(); mc.codebook = cbd; mcs.append(mc)
    outs = ops.CodeBatch(mcs, [1, -1, 0]).run_labels(_dev(label), reps, _dev(scale), n_half)
    _sync()
    for o, w in zip(outs, want):
        _assert_equal(o, w, 'CodeBatch.run_labels')


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,hw,c,channels_last', [(5, 1, 24, True), (5, 1, 24, False), (3, 7, 40, True), (3, 7, 40, False),
                                                  (65, 64, 256, True), (65, 64, 256, False)])
def test_code_apply(n, hw, c, channels_last, bf16):
    """mcgen_mc_apply: y = x code, one product: fp32 equals the float64 product rounded once, bf16 equals the
    round-to-nearest-even of that; [N, HW, C] and [N, C, HW]; HW = 1 is the [N, C] input; 65 x 64 x 256 elements wrap."""
    assert (n * hw * c > GRID_CAP) == (n == 65)
    gen = _gen('apply', n, hw, c, channels_last)
    shape = (n, hw, c) if channels_last else (n, c, hw)
    x = torch.randn(shape, generator=gen).to(_dt(bf16))
    code = (torch.rand(n, c, generator=gen) < 0.5).float() * (0.5 + torch.rand(n, c, generator=gen))
    y = _nan(n * hw * c, _dt(bf16))
    _ok(_lib().mcgen_mc_apply(_p(_dev(x)), _p(_dev(code)), _p(y), _dtc(bf16), n, hw, c, int(channels_last), _stream()), 'mc_apply')
    ref = x.double() * (code.double().view(n, 1, c) if channels_last else code.double().view(n, c, 1))
    ref = ref.float().double()
    _assert_equal(_out(y, n * hw * c, 'y').view(shape), R.round_bf16(ref) if bf16 else ref, 'mc_apply')


# ---- 5. compaction maps -------------------------------------------------------------------------------------------------
def _cmap_codes(c, gen):
    """Five rows: all zero, all active, one active channel at C - 1, random at rates 0.5 and 0.05 -- the random rows with
    one -0.0 (inactive) and one negative entry (active)."""
    code = torch.zeros(5, c)
    code[1] = 0.5 + torch.rand(c, generator=gen)
    code[2, c - 1] = 1.5
    for i, rate in ((3, 0.5), (4, 0.05)):
        code[i] = (torch.rand(c, generator=gen) < rate).float() * (0.5 + torch.rand(c, generator=gen))
        code[i, 1] = -0.0
        code[i, c // 2] = -0.75
    return code


def _launch_cmap(code):
    n, c = code.shape
    stride = _ops().cmap_stride(c)
    cm = torch.full((n * stride + GAP,), SENT16, dtype=torch.int16, device='cuda')
    _ok(_lib().mcgen_mc_cmap(_p(_dev(code)), n, c, _p(cm), _stream()), 'mc_cmap')
    flat = cm.cpu()
    assert bool((flat[n * stride:] == SENT16).all()), 'mc_cmap wrote past its records'
    return cm, flat[:n * stride].view(n, stride), stride


@pytest.mark.parametrize('c', [8, 32, 40, 72, 256, 2048])
def test_cmap_records(c):
    """mcgen_mc_cmap: cpos, cidx and cpre of every record equal small_ops_ref.cmap_record; the int16 words between the
    record's end and the stride keep their sentinel.  C = 2048 fills the 64 count slots of the kernel's LDS table."""
    code = _cmap_codes(c, _gen('cmap', c))
    _, cm, stride = _launch_cmap(code)
    nd = (c + 31) // 32
    end = 2 * c + 32 + 2 * (nd + 1)
    assert stride >= end and stride % 8 == 0
    for i in range(code.shape[0]):
        cpos, cidx, cpre = R.cmap_record(code[i])
        assert torch.equal(cm[i, :c].long(), cpos), f'cpos of row {i}'
        assert torch.equal(cm[i, c:2 * c + 32].long(), cidx), f'cidx of row {i}'
        assert torch.equal(cm[i, 2 * c + 32:end].contiguous().view(torch.int32).long(), cpre), f'cpre of row {i}'
        assert bool((cm[i, end:] == SENT16).all()), f'row {i}: wrote between the record and the stride'
    assert int((code[3] != 0).sum()) == int(R.cmap_record(code[3])[2][-1]) and code[3, c // 2] < 0


@pytest.mark.parametrize('c', [2056, 12])
def test_cmap_refusals(c):
    cm = torch.full((4 * (2 * c + 256),), SENT16, dtype=torch.int16, device='cuda')
    rc = _lib().mcgen_mc_cmap(_p(_dev(torch.ones(4, c))), 4, c, _p(cm), _stream())
    _refused(rc, 'mc_cmap: bad arguments (C a multiple of 8, at most 2048)')
    assert bool((cm == SENT16).all())


@pytest.mark.parametrize('group_n', [0, 1, 3])
@pytest.mark.parametrize('affine', [True, False])
@pytest.mark.parametrize('c', [8, 72, 256])
def test_affine_rows(c, affine, group_n):
    """mcgen_mc_affine over the maps of mcgen_mc_cmap, for Ccap = 8, the largest active count rounded up to 8, and C + 32:
    every entry is one product (or the code itself, or 0), compared for equality; slots past the active count are 0."""
    gen = _gen('affine', c, affine, group_n)
    n = 6
    code = torch.cat([_cmap_codes(c, gen), (0.5 + torch.rand(1, c, generator=gen)) * (torch.rand(1, c, generator=gen) < 0.5)])
    code = code.abs()                                     # (codes are non-negative where the affine rows are used)
    groups = n // group_n if group_n else 1
    scale = torch.randn(groups, c, generator=gen) if affine else None
    shift = torch.randn(groups, c, generator=gen) if affine else None
    cm, _, _ = _launch_cmap(code)
    most = int((code != 0).sum(1).max())
    for ccap in sorted({8, (most + 7) // 8 * 8, c + 32}):
        so, ho = _nan(n * ccap), _nan(n * ccap)
        _ok(_lib().mcgen_mc_affine(_p(_dev(scale)), _p(_dev(shift)), group_n, _p(_dev(code)), _p(cm), n, c, ccap, _p(so), _p(ho), _stream()),
            'mc_affine')
        rs, rh = R.mc_affine_rows(code, ccap, scale, shift, group_n)
        _assert_equal(_out(so, n * ccap, 'scale_out').view(n, ccap), rs.float().double(), f'mc_affine scale_out, Ccap = {ccap}')
        _assert_equal(_out(ho, n * ccap, 'shift_out').view(n, ccap), rh.float().double(), f'mc_affine shift_out, Ccap = {ccap}')
        if ccap == c + 32:
            assert bool((rs[:, c:] == 0).all())


def test_affine_refusals():
    c, n = 16, 3
    code = torch.ones(n, c, device='cuda')
    cm, _, _ = _launch_cmap(code.cpu())
    sc = torch.ones(c, device='cuda')
    so, ho = _nan(n * (c + 40)), _nan(n * (c + 40))
    lib = _lib()
    _refused(lib.mcgen_mc_affine(_p(sc), _p(sc), 0, _p(code), _p(cm), n, c, c + 40, _p(so), _p(ho), _stream()), 'mc_affine: bad arguments', so, ho)
    _refused(lib.mcgen_mc_affine(_p(sc), None, 0, _p(code), _p(cm), n, c, 8, _p(so), _p(ho), _stream()),
             'mc_affine: scale and shift go together', so, ho)


# ---- 6. one-hot indicator -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_lab32', [True, False])
@pytest.mark.parametrize('n,classes,reps', [(1, 1, 1), (24, 10, 3), (64, 1623, 1), (7, 100, 5)])
def test_onehot_rep(n, classes, reps, with_lab32):
    """mcgen_onehot_rep: F.one_hot(label).float() `reps` times; labels -1 and `classes` give an all-zero row and a lab32
    clamped to 0 and classes - 1; lab32 = NULL is accepted.  64 x 1623 entries wrap the 256-block grid."""
    assert (n * classes * reps > ONEHOT_GRID) == (classes == 1623)
    gen = _gen('onehot', n, classes, reps)
    label = torch.randint(0, classes, (n,), generator=gen)
    if n >= 4:
        label[1], label[2], label[3], label[0] = -1, classes, classes - 1, 0
    for lab in ([label] if n > 1 else [label, label - 1, label + 1]):
        out = _nan(reps * n * classes)
        lab32 = torch.full((reps * n + GAP,), -77, dtype=torch.int32, device='cuda') if with_lab32 else None
        _ok(_lib().mcgen_onehot_rep(_p(_dev(lab)), _p(out), _p(lab32), n, classes, reps, _stream()), 'onehot_rep')
        inside = (lab >= 0) & (lab < classes)
        want = F.one_hot(lab.clamp(0, classes - 1), classes).double() * inside.view(n, 1)
        _assert_equal(_out(out, reps * n * classes, 'indicator').view(reps, n, classes), want.expand(reps, n, classes), 'onehot_rep')
        if with_lab32:
            l32 = lab32.cpu()
            assert torch.equal(l32[:reps * n].long(), lab.clamp(0, classes - 1).repeat(reps)) and bool((l32[reps * n:] == -77).all())


# ---- 7. layout ----------------------------------------------------------------------------------------------------------
LAYOUT = [(1, 1, 1, 1, 8), (3, 3, 5, 7, 8), (2, 12, 4, 4, 16), (2, 16, 4, 4, 16), (130, 3, 32, 32, 8)]
TIES = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -1 - 2.0 ** -8, -1 - 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23]


def _nchw_input(n, c, h, w, gen):
    x = torch.randn(n, c, h, w, generator=gen)
    k = min(len(TIES), x.numel())
    x.view(-1)[:k] = torch.tensor(TIES[:k])
    x.view(-1)[-k:] = torch.tensor(TIES[:k])
    return x


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,c,h,w,cp', LAYOUT)
def test_layout_conversions(n, c, h, w, cp, bf16):
    """mcgen_nchw_to_nhwc: fp32 bit-exact, bf16 == round_bf16 (the input holds ties: 1 + 2^-8 -> 1, 1 + 3 2^-8 ->
    1 + 2^-6), padding channels exactly zero.  mcgen_nhwc_to_nchw: the inverse, from a source whose padding channels are
    NaN: none may reach the output.  The round trip is the identity on bf16 values.  130 x 32 x 32 x 8 elements wrap."""
    lib = _lib()
    assert (n * h * w * cp > GRID_CAP) == (n == 130)
    assert float(R.round_bf16(torch.tensor([TIES[0]], dtype=F64))) == 1.0 and float(R.round_bf16(torch.tensor([TIES[1]], dtype=F64))) == 1 + 2.0 ** -6
    gen = _gen('layout', n, c, h, w, cp)
    x = _nchw_input(n, c, h, w, gen)
    y = _nan(n * h * w * cp, _dt(bf16))
    _ok(lib.mcgen_nchw_to_nhwc(_p(_dev(x)), _p(y), _dtc(bf16), n, c, h, w, cp, _stream()), 'nchw_to_nhwc')
    want = torch.zeros(n, h, w, cp, dtype=F64)
    want[..., :c] = x.double().permute(0, 2, 3, 1)
    if bf16:
        want = R.round_bf16(want)
    got = _out(y, n * h * w * cp, 'nhwc').view(n, h, w, cp)
    _assert_equal(got, want, 'nchw_to_nhwc')
    assert bool((got[..., c:] == 0).all())
    # back: padding channels of the source are NaN
    src = want.clone()
    src[..., c:] = NAN
    src = _dev(src.to(_dt(bf16)))
    back = _nan(n * c * h * w)
    _ok(lib.mcgen_nhwc_to_nchw(_p(src), _p(back), _dtc(bf16), n, c, h, w, cp, _stream()), 'nhwc_to_nchw')
    _assert_equal(_out(back, n * c * h * w, 'nchw').view(n, c, h, w), want[..., :c].permute(0, 3, 1, 2), 'nhwc_to_nchw')
    # round trip through the wrappers on bf16 values
    xb = x.bfloat16().float()
    rt = _ops().to_nchw(_ops().to_nhwc(_dev(xb), _dt(bf16), cp), c)
    _sync()
    assert torch.equal(rt.cpu(), xb)


@pytest.mark.parametrize('c,cp', [(12, 8), (12, 12)])
def test_layout_refusals(c, cp):
    y = _nan(2 * 4 * 16)
    rc = _lib().mcgen_nchw_to_nhwc(_p(_dev(torch.ones(2, c, 2, 2))), _p(y), _L().F32, 2, c, 2, 2, cp, _stream())
    _refused(rc, 'nchw_to_nhwc: bad arguments', y)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('n,ho,wo,c', [(1, 1, 1, 8), (3, 2, 5, 24)])
def test_pool2_sum(n, ho, wo, c, bf16):
    """mcgen_pool2_sum on random values: (a + b) + (c + d), 2u sum |terms|; bf16 adds 2^-8 of the stored value."""
    gen = _gen('pool', n, ho, wo, c)
    x = torch.randn(n, 2 * ho, 2 * wo, c, generator=gen).to(_dt(bf16))
    y = _nan(n * ho * wo * c, _dt(bf16))
    _ok(_lib().mcgen_pool2_sum(_p(_dev(x)), _p(y), _dtc(bf16), n, ho, wo, c, _stream()), 'pool2_sum')
    ref, mag = R.pool2_sum(x)
    tol = 2 * U32 * mag
    if bf16:
        tol = tol + U16 * (ref.abs() + tol)
    _assert_within(_out(y, n * ho * wo * c, 'pooled').view(n, ho, wo, c), ref, tol, 'pool2_sum')


@pytest.mark.parametrize('n,ho,wo,c,bf16', [(3, 2, 5, 24, False), (3, 2, 5, 24, True), (33, 16, 16, 1024, True)])
def test_pool2_sum_exact(n, ho, wo, c, bf16):
    """Multiples of 1/4 in [-4, 4]: every 2x2 sum is a bf16 number (asserted from the reference), so both dtypes compare
    for equality.  (33, 16, 16, 1024) has 33 x 256 x 128 threads' worth of work against 4096 x 256: the loop wraps; it
    runs in bf16 only (fp32 would take 173 MB)."""
    assert (n * ho * wo * c // 8 > GRID_CAP) == (n == 33)
    x = R.pool_exact_input(n, 2 * ho, 2 * wo, c, R.seed_of('pool exact', n, ho, wo, c))
    ref = x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]      # exact in fp32: 7 bits at most
    R.assert_exact(R.sum_bits(16.0, 0.25), 'pool2_sum')
    assert R.sum_bits(16.0, 0.25) <= 8 and float(x.abs().max()) <= 4.0 and bool((x * 4 == torch.round(x * 4)).all())
    y = _nan(n * ho * wo * c, _dt(bf16))
    _ok(_lib().mcgen_pool2_sum(_p(_dev(x.to(_dt(bf16)))), _p(y), _dtc(bf16), n, ho, wo, c, _stream()), 'pool2_sum')
    got = y.float().cpu()
    assert bool(torch.isnan(got[-GAP:]).all()) and torch.equal(got[:-GAP].view(n, ho, wo, c), ref)


def test_pool2_sum_refusal():
    y = _nan(2 * 12)
    rc = _lib().mcgen_pool2_sum(_p(_dev(torch.ones(2, 2, 2, 12))), _p(y), _L().F32, 2, 1, 1, 12, _stream())
    _refused(rc, 'pool2_sum: bad arguments (C a multiple of 8)', y)
