"""csrc/pixelcnn_sample.hip at its own limits, against the float64 reference of px_sample_ref.py (pinned on the CPU by
test_px_sample_ref_cpu.py): logits at channel counts and map widths that pad, split or exactly fill the MFMA tiles, the
inverse-CDF draw at every code of logit vectors built to break a softmax scan, greedy ties, guard bands around every
buffer the launches write, and the host-side refusals."""
import re

import pytest
import torch

import px_sample_ref as R

pytestmark = pytest.mark.gpu

MODES = 10
DTYPES = [torch.float32, torch.bfloat16]
FORMS = ['mcpixelcnn', 'cpixelcnn']


def _labels(n, seed):
    """Seeded labels that include the first and the last mode (one sample: the last)."""
    lab = torch.randint(0, MODES, (n,), generator=torch.Generator().manual_seed(seed))
    lab[0], lab[-1] = 0, MODES - 1
    return lab.cuda()


def _last_conv(m):
    from mcgen_amd.engine_base import _unwrap
    return _unwrap(m.output_conv[-1])


# ---- (a) logits at edge widths --------------------------------------------------------------------------------------------
GEOMETRIES = [(8, 1, 10, 1, 1, 1),          # the smallest of everything; one layer: no ring, no x_h store, no residual
              (8, 2, 65, 17, 3, 5),         # Kq not a multiple of 16; two column workgroups, the second with one sample
              (24, 3, 100, 37, 4, 7),       # r16(C) = 32 != C, 2C = 48; 4 samples x 7 columns = 28 rows of a 32-row tile
              (40, 2, 33, 5, 2, 33),        # W >= 32: one sample per workgroup, three row tiles, the odd one alone
              (16, 4, 32, 33, 2, 16)]       # SR * W = 32 exactly
BOUND = {torch.float32: 1e-5, torch.bfloat16: 2e-2}


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('geo', GEOMETRIES, ids=lambda g: 'x'.join(map(str, g)))
def test_logits_at_edge_widths(geo, form, dtype):
    hidden, layers, kq, n, h, w = geo
    m = R.build(form, hidden, layers, kq, MODES, 'cuda', seed=hidden + kq).set_compute_dtype(dtype)
    sd = R.state(m)
    store = None if dtype == torch.float32 else dtype
    for lab in ([_labels(n, 3)] if n > 1 else [torch.tensor([0]).cuda(), torch.tensor([MODES - 1]).cuda()]):
        x = torch.zeros((n, h, w), dtype=torch.long, device='cuda')
        u = torch.rand((h * w, n), generator=torch.Generator().manual_seed(n + w)).cuda()
        out, lg = m.sample(lab, x=x, uniform=u, return_logits=True)
        assert out is x and lg.shape == (n, kq, h, w) and lg.dtype == torch.float32
        assert int(out.min()) >= 0 and int(out.max()) < kq
        ref = R.forward64(sd, out, lab, MODES, form == 'cpixelcnn', store=store)
        err = float((lg.double().cpu() - ref).abs().max() / ref.abs().max())
        print(f'logits {form} {geo} {str(dtype)[6:]}: {err:.3g} of max|ref| (bound {BOUND[dtype]:g})')
        assert err <= BOUND[dtype], err


# ---- (b) the draw, exactly ------------------------------------------------------------------------------------------------
def _draw_model(form, bias, dtype):
    """hidden 8, one layer; the last 1x1 has weight 0 and bias `bias`, so every position's logits are the bias."""
    m = R.build(form, 8, 1, bias.numel(), MODES, 'cuda', seed=bias.numel()).set_compute_dtype(dtype)
    with torch.no_grad():
        _last_conv(m).weight.zero_()
        _last_conv(m).bias.copy_(bias.cuda())
    return m


def _check_draw(form, name, kq, dtype):
    n, w = 37, 7                                                      # 37 samples: column workgroups of 16, 16 and 5
    bias = R.case_logits(name, kq)
    u, _ = R.probes(bias)
    positions = -(-u.numel() // n)
    h = -(-positions // w)
    uniform = torch.full((h * w * n,), 0.5)
    uniform[:u.numel()] = u
    m = _draw_model(form, bias, dtype)
    x = torch.zeros((n, h, w), dtype=torch.long, device='cuda')
    out, lg = m.sample(_labels(n, 5), x=x, uniform=uniform.view(h * w, n).cuda(), return_logits=True)
    assert torch.equal(lg.cpu(), bias[None, :, None, None].expand(n, kq, h, w))            # bit for bit, fp32 and bf16
    got = out.cpu().permute(1, 2, 0).reshape(-1)                                           # [position, sample], as uniform
    want, dist = R.inverse_cdf64(bias, uniform)
    probe = torch.arange(uniform.numel()) < u.numel()
    wrong = (got != want) & (probe | (dist >= R.MARGIN))              # the 0.5 padding counts where it is clear of a boundary
    print(f'draw {form} {name} {kq} {str(dtype)[6:]}: {u.numel()} probes over {h * w} positions, {int(wrong.sum())} wrong')
    assert not bool(wrong.any()), [(float(uniform[i]), int(got[i]), int(want[i])) for i in wrong.nonzero().flatten()[:8]]
    assert int(got.min()) >= 0 and int(got.max()) < kq


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('name,kq', R.DRAW_CASES)
def test_draw_equals_float64_inverse_cdf(name, kq, dtype):
    _check_draw('mcpixelcnn', name, kq, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_draw_equals_float64_inverse_cdf_conditional(dtype):
    _check_draw('cpixelcnn', 'gauss', 100, dtype)


# ---- (c) greedy ties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('kq,ties', [(512, (9, 13, 300)), (10, (2, 5))])
def test_greedy_takes_the_first_of_tied_maxima(kq, ties, dtype):
    """512 codes: 9 and 13 share a lane of the scan, 300 lies in another; 10 codes: one code per lane."""
    bias = -(torch.arange(kq) % 5).float() * 0.5
    bias[list(ties)] = 1.0
    m = _draw_model('mcpixelcnn', bias, dtype)
    x = torch.zeros((37, 2, 3), dtype=torch.long, device='cuda')
    out = m.sample(_labels(37, 7), x=x, greedy=True)
    assert bool((out == ties[0]).all()), out.unique().tolist()


# ---- (d) no store outside the buffers -------------------------------------------------------------------------------------
GUARD = 4096
SENTINEL = {torch.float32: 3.0, torch.bfloat16: 3.0, torch.int64: -7}


def _guarded(shape, dtype, inside):
    """A contiguous `shape` view filled with `inside`, GUARD sentinel elements on either side of it in one allocation."""
    numel = int(torch.Size(shape).numel())
    whole = torch.full((numel + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device='cuda')
    whole[GUARD:GUARD + numel] = inside
    return whole, whole[GUARD:GUARD + numel].view(shape)


def _intact(whole, numel=0):
    s = SENTINEL[whole.dtype]
    return bool((whole[:GUARD] == s).all()) and bool((whole[GUARD + numel:] == s).all())


def _descriptor(m, lab, dtype, n, h, w, uniform, inside=float('nan'), codes_inside=999):
    """The mcgen_px_sample_t pixelcnn_sampler.sample fills, with every buffer the launches write inside a guard band
    -> (P, {name: (whole allocation, view)}, tensors to keep alive)."""
    from mcgen_amd import _lib, ops, pixelcnn_sampler as S
    from mcgen_amd.engine_base import _unwrap
    c, n_layer = m.hidden_size, len(m.layers)
    hd, kq = _unwrap(m.output_conv[0]).out_channels, _last_conv(m).out_channels
    emb, wpack, ppack = S.pack(m, dtype)
    if S.conditional(m):
        mc = ops.cpx_gather_rows(torch.stack([L.class_cond_embedding.weight.detach() for L in m.layers]), lab)
    else:
        mc = S._code_rows(ops.CodeBatch(S.controllers(m)).run_labels(lab))
    bufs = {'codes': _guarded((n, h, w), torch.int64, codes_inside),
            'ov': _guarded((n_layer, n, 2, w, c), dtype, inside),
            'v2h': _guarded((n_layer, n, w, 2 * c), torch.float32, inside),
            'xh': _guarded((n_layer, n, w, c), dtype, inside),
            'logits': _guarded((n, h, w, kq), torch.float32, inside)}
    P = _lib.PxSample()
    P.codes, P.emb, P.w, P.p, P.mc = ops._p(bufs['codes'][1]), ops._p(emb), ops._p(wpack), ops._f32(ppack), ops._f32(mc)
    P.ov, P.v2h, P.xh = ops._p(bufs['ov'][1]), ops._f32(bufs['v2h'][1]), ops._p(bufs['xh'][1])
    P.uniform, P.logits = ops._f32(uniform), ops._f32(bufs['logits'][1])
    P.N, P.H, P.W, P.C, P.L, P.Kq, P.Hd, P.greedy = n, h, w, c, n_layer, kq, hd, 0
    return P, bufs, (emb, wpack, ppack, mc, uniform)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('form', FORMS)
def test_launches_write_inside_their_buffers(form, dtype):
    """17 samples of a 3x5 map at hidden 24: row workgroups of 6, 6 and 5 samples, column workgroups of 16 and 1.  The
    workspace starts as NaN: nothing is read before it is written."""
    from mcgen_amd import ops
    hidden, layers, kq, n, h, w = 24, 3, 100, 17, 3, 5
    m = R.build(form, hidden, layers, kq, MODES, 'cuda', seed=2).set_compute_dtype(dtype)
    lab = _labels(n, 9)
    uniform = torch.rand((h * w, n), generator=torch.Generator().manual_seed(4)).cuda()
    P, bufs, keep = _descriptor(m, lab, dtype, n, h, w, uniform)
    row, col = (ops.cpx_sample_row, ops.cpx_sample_col) if form == 'cpixelcnn' else (ops.px_sample_row, ops.px_sample_col)
    for i in range(h):
        row(P, i, dtype)
        for j in range(w):
            col(P, i, j, dtype)
    torch.cuda.synchronize()
    for name, (whole, view) in bufs.items():
        assert _intact(whole, view.numel()), f'a store outside {name}'
    x, lg = m.sample(lab, x=torch.zeros((n, h, w), dtype=torch.long, device='cuda'), uniform=uniform, return_logits=True)
    assert torch.equal(bufs['codes'][1], x)
    assert torch.equal(bufs['logits'][1].permute(0, 3, 1, 2), lg)
    del keep


# ---- (e) refusals before any launch ---------------------------------------------------------------------------------------
LDS_MAX = 160 * 1024


def _a16(x):
    return (x + 15) // 16 * 16


def _row_lds(w, c, esz):
    """RowLds::bytes of csrc/pixelcnn_sample.hip."""
    sr = 1 if w >= 32 else 32 // w
    return _a16(sr * 3 * (w + 6) * 4) + _a16(sr * 2 * (w + 2) * c * esz) + _a16(sr * w) * (2 * c + 16 // esz) * esz


def _col_lds(c, hd, kq, esz):
    """ColLds::bytes of csrc/pixelcnn_sample.hip."""
    pad = 16 // esz
    rows = (3 * c + pad, 2 * c + pad, c + pad, c, hd + pad)
    return sum(_a16(16 * r * esz) for r in rows) + 16 * kq * 4


@pytest.mark.parametrize('form', FORMS)
def test_refusals_before_any_launch(form, monkeypatch):
    from mcgen_amd import _lib, ops
    dtype = torch.float32
    m = R.build(form, 8, 1, 10, MODES, 'cuda', seed=6)
    uniform = torch.full((1, 1), 0.5, device='cuda')
    P, bufs, keep = _descriptor(m, torch.tensor([3]).cuda(), dtype, 1, 1, 1, uniform, inside=SENTINEL[dtype],
                             codes_inside=SENTINEL[torch.int64])
    pre = 'cpx' if form == 'cpixelcnn' else 'px'
    row, col = getattr(ops, pre + '_sample_row'), getattr(ops, pre + '_sample_col')

    def refused(call, message, **fields):
        old = {k: getattr(P, k) for k in fields}
        for k, v in fields.items():
            setattr(P, k, v)
        try:
            with pytest.raises(_lib.McgenError, match=message) as e:
                call()
        finally:
            for k, v in old.items():
                setattr(P, k, v)
        torch.cuda.synchronize()
        for name, (whole, _) in bufs.items():
            assert bool((whole == SENTINEL[whole.dtype]).all()), f'{name} was written by a refused launch'
        return str(e.value)

    # a position outside the map
    refused(lambda: row(P, 1, dtype), rf'{pre}_sample_row: row 1 outside \[0, 1\)')
    refused(lambda: row(P, -1, dtype), r'row -1 outside')
    refused(lambda: col(P, 0, 1, dtype), rf'{pre}_sample_col: bad position \(0, 1\)')
    refused(lambda: col(P, 1, 0, dtype), r'bad position \(1, 0\)')
    refused(lambda: col(P, 0, -1, dtype), r'bad position \(0, -1\)')
    # no uniforms
    refused(lambda: col(P, 0, 0, dtype), r'bad position \(0, 0\) or no uniforms', uniform=None)
    # a channel count that is no multiple of 8
    refused(lambda: row(P, 0, dtype), r'px_sample: bad shape .* C 12 ', C=12)
    refused(lambda: col(P, 0, 0, dtype), r'px_sample: bad shape .* C 12 ', C=12)
    # a dtype id the library does not know
    monkeypatch.setattr(ops, '_dt', lambda dt: 2)
    refused(lambda: row(P, 0, dtype), r'px_sample: unknown dtype 2')
    refused(lambda: col(P, 0, 0, dtype), r'px_sample: unknown dtype 2')
    monkeypatch.undo()
    # more LDS than a workgroup has: the smallest Kq / W past the limit by the structs' own formulas
    kq = next(k for k in range(1, 1 << 16) if _col_lds(8, 512, k, 4) > LDS_MAX)
    assert _col_lds(8, 512, kq - 1, 4) <= LDS_MAX
    msg = refused(lambda: col(P, 0, 0, dtype), r'bytes of LDS for C 8 Hd 512 Kq', Kq=kq)
    assert int(re.search(r'(\d+) bytes of LDS', msg).group(1)) == _col_lds(8, 512, kq, 4)
    w = next(v for v in range(32, 1 << 16) if _row_lds(v, 8, 4) > LDS_MAX)
    assert _row_lds(w - 1, 8, 4) <= LDS_MAX
    msg = refused(lambda: row(P, 0, dtype), r'bytes of LDS for W', W=w)
    assert int(re.search(r'(\d+) bytes of LDS', msg).group(1)) == _row_lds(w, 8, 4)
    del keep
