"""The split-K slab reduce (reduce_job in csrc/wgrad.hip) on its own: mcgen_wgrad_reduce and mcgen_wgrad_reduce_batch
on synthetic slabs laid out by weight_image_ref.slab_layout, against weight_image_ref.reduce in float64.  No
convolution is launched.

Two kinds of slab:

- int: live entries are integers, |v| <= 512, alpha and row_scale are powers of two in [1/4, 4], previous gradient
  contents are integers, |p| <= 16.  A sum of at most 4 * 131 such entries is an integer below 2^19, the scale shifts
  its exponent, and adding the previous value keeps the result within 24 significant bits -- every partial sum, in ANY
  order and with or without fused multiply-adds, is exact in fp32.  The result must equal the reference bit for bit.
- rand: live entries are randn, alpha and row_scale arbitrary.  With u = 2^-24 (fp32 unit roundoff): `splits` terms summed
  by fp32 additions in any order (lane split, unrolled groups, butterfly) carry an error of at most (splits - 1) u times
  the sum of their magnitudes; ra = alpha * row_scale is one rounding, s * ra a second, adding the previous value a third
  (a fused multiply-add would save one).  To first order
      |got - ref| <= (splits + 3) u (|alpha row_scale| sum_abs + |previous|)
  per element; the bias gradient sums 4 * splits rows: (4 splits + 3) u.  Nothing here was tuned to what the kernel gives,
  and the bound does not depend on the summation order.

Every dead slab entry (rows >= Cout, columns >= Cin, the padding of cin_slab, compact columns of taps >= k * k, bias
columns >= Cout) is NaN in both kinds: the outputs have to be finite all the same.  Gradients carry a sentinel tail of 64
floats that must survive, and with accumulate = 0 they start as NaN, so every in-range element has to be written."""
import numpy as np
import pytest
import torch

import weight_image_ref as R

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
TAIL = 64
SENTINEL = -12345.5


def _case(splits, cout, cout_w, cin, cin_slab, ks, *, perm=1, rs=False, acc=0, bias=0, win=None, tapcols=0):
    return dict(splits=splits, Cout=cout, Cout_w=cout_w, Cin=cin, cin_slab=cin_slab, ksize=ks, row_perm=perm, row_scale=rs,
                accumulate=acc, bias=bias, win=win, tapcols=tapcols)


# Each value the reduce treats differently appears at least once (not the full product); a case stays under ~300 k
# slab floats.  splits: both sides of every reduce_lanes boundary (8 / 16 / 32 / 64) and lane trip counts with every
# remainder the four-way unrolled loop leaves; `win` = (tap0, ntap_out).
CASES = [
    _case(1, 3, 16, 3, 0, 1),
    _case(7, 24, 32, 8, 0, 3, perm=2, rs=True, acc=1, bias=1, win=(0, 6)),
    _case(8, 24, 32, 40, 48, 3, bias=2, win=(3, 2)),
    _case(9, 130, 144, 40, 0, 1, perm=2, rs=True, bias=1),
    _case(16, 3, 16, 72, 96, 3, rs=True, acc=1, win=(4, 1)),
    _case(17, 24, 32, 3, 8, 3, rs=True, acc=1, bias=2, win=(8, 1)),
    _case(32, 130, 144, 8, 0, 1, bias=1),
    _case(33, 24, 32, 40, 0, 1, rs=True, acc=1),
    _case(64, 32, 32, 40, 0, 1, perm=16, rs=True, bias=1),
    _case(65, 3, 16, 3, 0, 3, acc=1, bias=2, win=(0, 0)),
    _case(131, 24, 32, 8, 0, 1, perm=2, rs=True, acc=1, bias=1),
    _case(2, 130, 144, 72, 0, 3, acc=1, bias=1),
    # the image layer's compact slabs: 72 live columns in 96 (3x3), 8 in 32 (1x1)
    _case(17, 128, 128, 3, 8, 3, bias=2, tapcols=1),
    _case(9, 24, 32, 8, 0, 1, rs=True, acc=1, bias=1, tapcols=1),
    _case(65, 24, 32, 1, 8, 3, acc=1, tapcols=1),
    _case(64, 128, 128, 8, 0, 1, bias=1, tapcols=1),
]
IDS = ['s{splits}-co{Cout}of{Cout_w}-ci{Cin}of{cin_slab}-k{ksize}-p{row_perm}-rs{row_scale:d}-a{accumulate}-b{bias}-w{win}-t{tapcols}'
       .format(**c) for c in CASES]


def test_case_list_covers_what_the_issue_names():
    have = lambda k: {c[k] for c in CASES}
    assert have('splits') >= {1, 7, 8, 9, 16, 17, 32, 33, 64, 65, 131}
    assert {(c['Cout'], c['Cout_w']) for c in CASES} >= {(3, 16), (24, 32), (130, 144)}
    assert {c['Cin'] for c in CASES if not c['tapcols']} >= {3, 8, 40, 72} and have('cin_slab') >= {0, 8, 48, 96}
    assert have('ksize') == {1, 3} and have('row_perm') == {1, 2, 16} and have('row_scale') == {False, True}
    assert have('accumulate') == {0, 1} and have('bias') == {0, 1, 2}
    assert have('win') >= {None, (0, 0), (0, 6), (3, 2), (4, 1), (8, 1)}
    assert {(c['Cin'], c['ksize'], c['Cout']) for c in CASES if c['tapcols']} >= {(3, 3, 128), (8, 1, 24), (1, 3, 24), (8, 1, 128)}
    for c in CASES:
        shape = R.slab_layout(c['Cout_w'], c['Cin'], c['cin_slab'], c['ksize'], c['tapcols'], c['Cout'])[0]
        assert c['splits'] * int(np.prod(shape)) <= 320_000, c


def _lib():
    from mcgen_amd import _lib as L
    return L.load()


class Job:
    """Host data, device buffers and the float64 reference of one case."""

    def __init__(self, c, kind, seed):
        self.c = c
        rng = np.random.default_rng(seed)
        splits, Cout, Cin, Cout_w = c['splits'], c['Cout'], c['Cin'], c['Cout_w']
        shape, co, ci, tap = R.slab_layout(Cout_w, Cin, c['cin_slab'], c['ksize'], c['tapcols'], Cout)
        live = co >= 0
        draw = (lambda s: rng.integers(-512, 513, s).astype(np.float32)) if kind == 'int' else \
               (lambda s: rng.standard_normal(s).astype(np.float32))
        prev = (lambda s: rng.integers(-16, 17, s).astype(np.float32)) if kind == 'int' else \
               (lambda s: rng.standard_normal(s).astype(np.float32))
        slabs = draw((splits,) + shape)
        slabs[:, ~live] = np.nan
        self.tap0, self.ntap_out = c['win'] if c['win'] else (0, 0)
        nout = self.ntap_out if self.ntap_out > 0 else c['ksize'] ** 2
        if kind == 'int':
            self.alpha = float(2.0 ** rng.integers(-2, 3))
            rs = (2.0 ** rng.integers(-2, 3, Cout)).astype(np.float32) if c['row_scale'] else None
        else:
            self.alpha = R.f32(0.37)
            rs = (rng.uniform(0.3, 3.0, Cout) * rng.choice([-1.0, 1.0], Cout)).astype(np.float32) if c['row_scale'] else None
        self.n = Cout * Cin * nout
        grad0 = prev(self.n) if c['accumulate'] else np.full(self.n, np.nan, np.float32)
        bslabs = bias0 = None
        if c['bias']:
            bslabs = draw((splits * 4, Cout_w))
            bslabs[:, Cout:] = np.nan
            bias0 = [prev(Cout) if c['accumulate'] else np.full(Cout, np.nan, np.float32) for _ in range(c['bias'])]
        self.ref = R.reduce(slabs, Cout, Cin, c['ksize'], Cout_w, cin_slab=c['cin_slab'], tapcols=c['tapcols'], alpha=self.alpha,
                            row_scale=rs, row_perm=c['row_perm'], accumulate=grad0 if c['accumulate'] else None,
                            tap0=self.tap0, ntap_out=self.ntap_out, bias_slabs=bslabs,
                            bias_accumulate=bias0[0] if c['bias'] and c['accumulate'] else None)
        self.ref2 = None
        if c['bias'] == 2:                                  # the second destination has previous contents of its own
            self.ref2 = R.reduce(slabs, Cout, Cin, c['ksize'], Cout_w, cin_slab=c['cin_slab'], tapcols=c['tapcols'], alpha=self.alpha,
                                 row_scale=rs, row_perm=c['row_perm'], tap0=self.tap0, ntap_out=self.ntap_out, bias_slabs=bslabs,
                                 bias_accumulate=bias0[1] if c['accumulate'] else None)['bias']
        self.scale_abs = abs(self.alpha) * (np.abs(rs.astype(np.float64)) if rs is not None else np.ones(Cout))
        self.prev_abs = np.abs(grad0.astype(np.float64)).reshape(Cout, Cin, nout) if c['accumulate'] else np.zeros((Cout, Cin, nout))
        self.bias_prev_abs = [np.abs(b.astype(np.float64)) if c['accumulate'] else np.zeros(Cout) for b in (bias0 or [])]
        self.host = (slabs, grad0, bslabs, bias0, rs)
        self.upload()

    def upload(self):
        slabs, grad0, bslabs, bias0, rs = self.host
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        tailed = lambda a: dev(np.concatenate([a, np.full(TAIL, SENTINEL, np.float32)]))
        self.slabs, self.grad = dev(slabs), tailed(grad0)
        self.bias_slabs = dev(bslabs) if bslabs is not None else None
        self.bias_grads = [tailed(b) for b in (bias0 or [])]
        self.row_scale = dev(rs) if rs is not None else None

    def args(self):
        c, p = self.c, (lambda t: None if t is None else t.data_ptr())
        bg = self.bias_grads + [None, None]
        return (p(self.slabs), c['splits'], p(self.grad), c['Cout'], c['Cin'], c['ksize'], c['Cout_w'], c['row_perm'], self.alpha,
                c['accumulate'], p(self.bias_slabs), p(bg[0]), p(bg[1]), p(self.row_scale), c['cin_slab'], c['tapcols'],
                self.tap0, self.ntap_out)

    def run(self):
        rc = _lib().mcgen_wgrad_reduce(*self.args(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _lib().mcgen_last_error()
        torch.cuda.synchronize()

    def fill(self, a):
        c, p = self.c, (lambda t: None if t is None else t.data_ptr())
        bg = self.bias_grads + [None, None]
        a.slabs, a.grad, a.bias_slabs, a.bias_grad, a.bias_grad2 = p(self.slabs), p(self.grad), p(self.bias_slabs), p(bg[0]), p(bg[1])
        a.splits, a.Cout, a.Cin, a.ksize, a.Cout_w = c['splits'], c['Cout'], c['Cin'], c['ksize'], c['Cout_w']
        a.row_perm, a.accumulate, a.alpha, a.row_scale = c['row_perm'], c['accumulate'], self.alpha, p(self.row_scale)
        a.cin_slab, a.tapcols, a.tap0, a.ntap_out = c['cin_slab'], c['tapcols'], self.tap0, self.ntap_out

    def results(self):
        """(grad, [bias grads]) as float64 numpy, after checking the sentinel tails."""
        out = []
        for t, n in [(self.grad, self.n)] + [(b, self.c['Cout']) for b in self.bias_grads]:
            h = t.cpu().numpy()
            assert (h[n:] == np.float32(SENTINEL)).all() and h.size == n + TAIL, 'the sentinel tail was written'
            out.append(h[:n].astype(np.float64))
        return out[0].reshape(self.ref['grad'].shape), out[1:]

    def check(self, kind):
        grad, biases = self.results()
        assert np.isfinite(grad).all(), 'a dead (NaN) slab entry reached the gradient, or an element was not written'
        refs = [self.ref['bias'], self.ref2][:len(biases)]
        for b in biases:
            assert np.isfinite(b).all(), 'a dead (NaN) bias column reached the bias gradient, or an element was not written'
        if kind == 'int':
            bad = np.argwhere(grad != self.ref['grad'])
            assert bad.size == 0, f'{len(bad)} elements differ, first (row, ci, tap) = {bad[0]}: got {grad[tuple(bad[0])]}, want {self.ref["grad"][tuple(bad[0])]}'
            for b, r in zip(biases, refs):
                assert np.array_equal(b, r), (b, r)
            return
        splits = self.c['splits']
        bound = (splits + 3) * U32 * (self.scale_abs[:, None, None] * self.ref['sum_abs'] + self.prev_abs)
        err = np.abs(grad - self.ref['grad'])
        print(f'grad: worst error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}')
        assert (err <= bound).all(), f'worst error / bound = {np.max(err / np.maximum(bound, 1e-300))}'
        for b, r, pa in zip(biases, refs, self.bias_prev_abs):
            bb = (4 * splits + 3) * U32 * (self.scale_abs * self.ref['bias_sum_abs'] + pa)
            be = np.abs(b - r)
            print(f'bias: worst error / bound = {np.max(be / np.maximum(bb, 1e-300)):.3f}')
            assert (be <= bb).all(), f'bias: worst error / bound = {np.max(be / np.maximum(bb, 1e-300))}'


@pytest.mark.parametrize('kind', ['int', 'rand'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_reduce_matches_the_reference(case, kind):
    job = Job(case, kind, seed=1000 + CASES.index(case))
    job.run()
    job.check(kind)


@pytest.mark.parametrize('case', [CASES[4], CASES[8], CASES[10], CASES[12]], ids=lambda c: f's{c["splits"]}')
def test_the_same_call_twice_gives_the_same_bits(case):
    job = Job(case, 'rand', seed=7)
    job.run()
    first = [job.grad.clone()] + [b.clone() for b in job.bias_grads]
    job.upload()                                            # (accumulating cases start from the same previous values)
    job.run()
    for a, b in zip(first, [job.grad] + job.bias_grads):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('kind', ['int', 'rand'])
def test_batch_of_37_jobs_equals_the_single_calls(kind):
    from mcgen_amd import _lib as L
    n = 37
    assert n > L.CONSTANTS['MCGEN_WREDUCE_MAX']             # two launches
    order = [CASES[(5 * i + 3) % len(CASES)] for i in range(n)]
    single = [Job(c, kind, seed=50 + i) for i, c in enumerate(order)]
    for j in single:
        j.run()
    batch = [Job(c, kind, seed=50 + i) for i, c in enumerate(order)]
    table = (L.WReduce * n)()
    for a, j in zip(table, batch):
        j.fill(a)
    rc = _lib().mcgen_wgrad_reduce_batch(table, n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib().mcgen_last_error()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(single, batch)):
        for x, y in zip([a.grad] + a.bias_grads, [b.grad] + b.bias_grads):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f'job {i}: {order[i]}'
        b.check(kind)


@pytest.mark.parametrize('change, text', [
    (dict(win=(7, 3)), 'bad tap window'),
    (dict(win=(-1, 2)), 'bad tap window'),
    (dict(row_perm=5), 'row_perm must divide Cout'),
    (dict(cin_slab=4), 'cin_slab is the (padded) channel count'),
    (dict(tapcols=1, Cin=9, cin_slab=0), 'tapcols slabs hold 8-channel layers'),
], ids=['window-past-the-end', 'window-negative', 'row_perm', 'cin_slab', 'tapcols'])
def test_host_checks_refuse_what_the_header_says(change, text):
    """Refused before any launch: the gradient keeps its NaN fill."""
    job = Job(_case(2, 24, 32, 8, 0, 3), 'int', seed=3)
    before = job.grad.clone()
    job.c = dict(job.c, **{k: v for k, v in change.items() if k != 'win'})
    if 'win' in change:
        job.tap0, job.ntap_out = change['win']
    rc = _lib().mcgen_wgrad_reduce(*job.args(), torch.cuda.current_stream().cuda_stream)
    assert rc != 0
    msg = _lib().mcgen_last_error().decode()
    assert msg.startswith('wgrad_reduce:') and text in msg, msg
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), job.grad.view(torch.int32))
