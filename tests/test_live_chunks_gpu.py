"""mcgen_conv_t.wlive: per-mode launches stop their K loops at the live 32-channel chunks of the tile's weight set.

Six weight sets over a compacted pitch of 96 channels (3 chunks) whose live channel counts sit on every chunk boundary:
0, 32, 33, 64, 65, 96 -> 0, 1, 2, 2, 3, 3 chunks.  Image i reads set i % 6, so neighbouring tiles belong to different
sets.  A two-segment launch gives its 1x1 shortcut the counts in reverse order (96 .. 0), so that the two segments of one
tile stop at different chunks and the tail's weight tiles must be found behind the WHOLE 3x3 image, not behind the chunks
the tile multiplied.  Per route (the three software-pipelined tiles at the smallest batch that reaches them, each with
one and with two segments, and the image head):

    a  with the table, output and BatchNorm partial sums are bit-identical to the same launch without it;
    b  the output matches a float64 masked convolution computed on the CPU within the kernel-level bf16 bound
       (4e-3 max|ref| + 1e-2 |ref|, and never more than 4e-3 max|ref| + 1e-2);
    c  with 3e30 written into the activation columns at and beyond 32 * chunks of every image and 1.0 into the weight
       columns there, the launch with the table still returns (a)'s bits: the bound is honoured, not just carried;
    d  table entries far beyond the pitch are clamped to it (and negative ones to 0).

The CPU test (e) checks the tables GeneratorEngine builds against numpy on sampled codebooks, before and after `create`.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

PITCH = 96
LIVE = [0, 32, 33, 64, 65, 96]                     # live channels of the six sets (segment 0); segment 1: reversed
BIG = 3.0e30


def _ops():
    from mcgen_amd import ops
    return ops


def _q(x):
    return x.to(torch.bfloat16).float()


def _chunks(live):
    return [(v + 31) // 32 for v in live]


def _mask(live):
    return (torch.arange(PITCH).view(1, -1) < torch.tensor(live).view(-1, 1)).float()          # [sets, PITCH]


def _edges(x):
    """Large positive entries next to every chunk edge and in the last column: a dropped or doubled column shows."""
    x = x.clone()
    for ch in (0, 31, 32, 63, 64, PITCH - 1):
        x[1::2, ch] = x[1::2, ch].abs() * 8 + 8
    return x


def _launch(ops, segs, sets, cout, bias, label, table, **kw):
    ops.TILE_LOG, ops.KERNEL_LOG = [], []
    try:
        y, st = ops.conv_fused(segs, sets.view(-1), cout, bias=bias, wsel=label, wlive=table, **kw)
        return y, st, list(ops.TILE_LOG), list(ops.KERNEL_LOG)
    finally:
        ops.TILE_LOG = ops.KERNEL_LOG = None


def _poison_x(x, chunks, label):
    """x [N, PITCH, H, W] with BIG in the columns at and beyond 32 * chunks[label[i]] of image i."""
    x = x.clone()
    for i in range(x.shape[0]):
        x[i, 32 * chunks[int(label[i])]:] = BIG
    return x


def _assert_bound(got, ref, what):
    got, ref = got.double().cpu(), ref.double()
    mx = float(ref.abs().max())
    err = (got - ref).abs()
    tol = 4e-3 * mx + 1e-2 * ref.abs().clamp(max=1.0)
    print(f'{what}: max err {float(err.max()):.3e}, max |ref| {mx:.3e}, smallest margin {float((tol - err).min()):.3e}')
    assert bool((err <= tol).all()), f'{what}: {int((err > tol).sum())} of {err.numel()} beyond the bound, max err {float(err.max()):.3e}'


class _Case:
    """Operands of one launch: clean and poisoned activations / weight sets, tables, the float64 reference on `sub`."""

    def __init__(self, n, h, cout, two_seg, head=False):
        ops = _ops()
        dt = torch.bfloat16
        g = torch.Generator().manual_seed(4201 + 7 * n + h + cout + int(two_seg))
        sets = len(LIVE)
        self.n, self.h, self.cout, self.two_seg = n, h, cout, two_seg
        self.label = torch.arange(n) % sets
        live = [LIVE] + ([LIVE[::-1]] if two_seg else [])
        self.chunks = [_chunks(v) for v in live]
        self.table = torch.tensor(self.chunks, dtype=torch.int32).t().contiguous().cuda()           # [sets, segments]
        x = _edges(torch.randn(n, PITCH, h, h, generator=g))
        sc, sh = torch.rand(n, PITCH, generator=g) + 0.5, torch.randn(n, PITCH, generator=g) * 0.3
        w3 = torch.randn(cout, PITCH, 3, 3, generator=g) * 0.05
        self.bias = torch.randn(cout, generator=g)
        xs, ws, ks = [x], [w3], [3]
        if two_seg:
            xs.append(_edges(torch.randn(n, PITCH, h // 2, h // 2, generator=g)))
            ws.append(torch.randn(cout, PITCH, 1, 1, generator=g) * 0.1)
            ks.append(1)

        def segments(poison):
            out = []
            for s, xx in enumerate(xs):
                xt = ops.to_nhwc((_poison_x(xx, self.chunks[s], self.label) if poison else xx).cuda(), dt)
                assert xt.shape[-1] == PITCH
                out.append(ops.Seg(xt, scale=sc.cuda(), shift=sh.cuda(), relu=True, group_n=1) if s == 0 else
                           ops.Seg(xt, ksize=1, ups=True))
            return out

        def weight_sets(poison):
            per = []
            for m in range(sets):
                parts = []
                for s, w in enumerate(ws):
                    wm = w * _mask(live[s])[m].view(1, -1, 1, 1)                     # zero columns behind the live ones
                    if poison:
                        wm[:, 32 * self.chunks[s][m]:] = 1.0
                    parts.append(ops.prep_weight(wm.cuda(), dt))
                per.append(torch.cat(parts))
            return torch.stack(per).contiguous()
        self.segs, self.segs_bad = segments(False), segments(True)
        self.sets, self.sets_bad = weight_sets(False), weight_sets(True)
        # float64 reference of every image
        ref = torch.empty(n, cout, h, h, dtype=torch.float64)
        for k, i in enumerate(range(n)):
            m = int(self.label[i])
            a = _q(torch.relu(_q(x[i:i + 1]) * sc[i].view(1, -1, 1, 1) + sh[i].view(1, -1, 1, 1)))
            r = F.conv2d(a.double(), _q(w3 * _mask(live[0])[m].view(1, -1, 1, 1)).double(), self.bias.double(), padding=1)
            if two_seg:
                up = _q(xs[1][i:i + 1]).repeat_interleave(2, 2).repeat_interleave(2, 3)
                r = r + F.conv2d(up.double(), _q(ws[1] * _mask(live[1])[m].view(1, -1, 1, 1)).double())
            ref[k] = r[0]
        self.ref = torch.tanh(ref) if head else ref


def _check(c, tile=None, form=0, **kw):
    ops = _ops()
    lab, bias = c.label.to(torch.int32).cuda(), c.bias.cuda()
    stats = kw.get('stats_mode', 0) != 0
    y0, st0, tiles, forms = _launch(ops, c.segs, c.sets, c.cout, bias, lab, None, **kw)
    assert forms == [form] and (tile is None or tiles == [tile]), (tiles, forms)
    # a: the table changes nothing
    y1, st1, _, forms = _launch(ops, c.segs, c.sets, c.cout, bias, lab, c.table, **kw)
    assert forms == [form]
    assert torch.equal(y1, y0), 'a: output with the table differs from the launch without it'
    assert not stats or torch.equal(st1, st0), 'a: BatchNorm partial sums differ'
    # b: float64 masked convolution
    _assert_bound(ops.to_nchw(y1, c.cout), c.ref, 'b')
    # c: the chunks behind the bound are not touched
    y2, st2, _, _ = _launch(ops, c.segs_bad, c.sets_bad, c.cout, bias, lab, c.table, **kw)
    assert bool(torch.isfinite(y2.float()).all()), 'c: a poisoned chunk reached the accumulators'
    assert torch.equal(y2, y0), 'c: output changed with poisoned columns behind the live chunks'
    assert not stats or torch.equal(st2, st0), 'c: BatchNorm partial sums changed'
    # d: clamped from above and from below
    big = torch.full_like(c.table, 1 << 20)
    y3, st3, _, _ = _launch(ops, c.segs, c.sets, c.cout, bias, lab, big, **kw)
    assert torch.equal(y3, y0) and (not stats or torch.equal(st3, st0)), 'd: an entry beyond the pitch is not clamped'
    neg = torch.where(c.table == 0, torch.full_like(c.table, -5), c.table)
    y4, _, _, _ = _launch(ops, c.segs, c.sets, c.cout, bias, lab, neg, **kw)
    assert torch.equal(y4, y0), 'd: a negative entry does not count as 0'


PP_CASES = [
    # N, H, Cout, tile
    (64, 32, 160, (256, 256)),
    (256, 16, 160, (256, 256)),
    (128, 16, 160, (128, 256)),
    (64, 32, 128, (256, 128)),
]


@pytest.mark.gpu
@pytest.mark.parametrize('two_seg', [False, True])
@pytest.mark.parametrize('n,h,cout,tile', PP_CASES)
def test_pp_tiles_stop_at_the_live_chunks(n, h, cout, tile, two_seg):
    _check(_Case(n, h, cout, two_seg), tile=tile, stats_mode=1)


@pytest.mark.gpu
def test_image_head_stops_at_the_live_chunks():
    """conv_head_kernel: 32x32 maps, 3 output channels of pitch 8, two images per set."""
    ops = _ops()
    c = _Case(12, 32, 3, False, head=True)
    _check(c, form=5, tanh=True)
    # the paired output layout takes the same kernel: its second halves are the plain launch's images
    lab = c.label.to(torch.int32).cuda()
    pair = torch.zeros(24, 32, 32, 8, dtype=torch.bfloat16, device='cuda')
    ops.conv_fused(c.segs_bad, c.sets_bad.view(-1), 3, bias=c.bias.cuda(), tanh=True, wsel=lab, wlive=c.table, out=pair, y_group=6)
    y0, _ = ops.conv_fused(c.segs, c.sets.view(-1), 3, bias=c.bias.cuda(), tanh=True, wsel=lab)
    assert torch.equal(pair.view(2, 12, 32, 32, 8)[:, 6:].reshape(12, 32, 32, 8), y0)


@pytest.mark.gpu
def test_table_needs_weight_sets_and_its_shape():
    ops = _ops()
    c = _Case(64, 32, 160, False)
    lab = c.label.to(torch.int32).cuda()
    with pytest.raises(Exception):                          # one column per segment
        ops.conv_fused(c.segs, c.sets.view(-1), 160, wsel=lab, wlive=torch.zeros(6, 2, dtype=torch.int32, device='cuda'))
    with pytest.raises(Exception):                          # without weight sets
        ops.conv_fused(c.segs, c.sets[5].contiguous(), 160, wlive=c.table)


@pytest.mark.gpu
def test_clamped_labels_index_the_tables():
    """mcgen_onehot_rep: the int32 labels (what wsel indexes weight sets and live-chunk tables with) are clamped into
    [0, classes) as mcgen_mc_gather_batch clamps the codebook row; the indicator row of such a label stays all zero."""
    ops = _ops()
    label = torch.tensor([0, 9, -3, 10, 1 << 40, 4], dtype=torch.int64, device='cuda')
    lab32 = torch.full((12,), -77, dtype=torch.int32, device='cuda')
    ind = ops.onehot_rep(label, 10, 2, lab32=lab32)
    assert lab32.cpu().tolist() == [0, 9, 0, 9, 9, 4] * 2
    want = torch.zeros(6, 10)
    want[0, 0] = want[1, 9] = want[5, 4] = 1.0
    assert torch.equal(ind.cpu(), want.repeat(2, 1))


# ---- e: the tables the engine builds (no GPU) ---------------------------------------------------------------------------
def _cpu_generator(width):
    from mcgen_amd import models
    from mcgen_amd.config import cfg, process_control
    cfg.update(data_name='CIFAR10', model_name='mcgan', device='cpu')
    cfg.pop('classes_size', None)
    process_control()
    cfg['gan']['generator_hidden_size'] = [width] * 4
    torch.manual_seed(1234 + width)
    return models.mcgan().generator


def _expected_tables(eng):
    """numpy: per per-mode image of the plan, ceil(live / 32) of the controller behind each segment's kmap."""
    plan, out = eng._plan(), {}
    modes = eng._codes.mcs[0].codebook.shape[0]
    for name, _ in plan.buffers:
        jobs = [j for j in plan.jobs if j.buffer == name]
        if not any(j.kmap for j in jobs):
            continue
        cols = []
        for j in jobs[:len(jobs) // modes]:
            if j.kmap:
                live = (eng._codes.mcs[j.kmap[0]].codebook.numpy() != 0).sum(1)
                cols.append(np.ceil(live / 32).astype(np.int64))
            else:
                cols.append(None)
        out[name] = cols
    return out


@pytest.mark.parametrize('width', [256, 128])
def test_engine_tables_are_the_live_chunks_of_the_codebooks(width):
    from mcgen_amd.config import cfg
    from mcgen_amd.gan_engine import GeneratorEngine, LIVE_ALL
    from mcgen_amd.models import utils as mutils
    try:
        gen = _cpu_generator(width)
        eng = GeneratorEngine(gen, torch.bfloat16)
        assert eng._codes.mcs[0].codebook.shape == (10, width)

        def check():
            got, want = eng.live_chunks(), _expected_tables(eng)
            assert set(got) == set(want) and {'b1.w2sm', 'b2.w1m', 'b2.w2sm', 'headm'} <= set(got), sorted(got)
            for name, cols in want.items():
                t = got[name]
                assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (10, len(cols))
                for s, col in enumerate(cols):
                    assert np.array_equal(t[:, s].numpy(), col if col is not None else np.full(10, LIVE_ALL)), (name, s)
            return got
        first = check()
        assert eng.live_chunks() is first                                   # cached per plan
        # block 1's shortcut reads x dense (block 0 does not store compacted): its column keeps every chunk
        assert bool((first['b1.w2sm'][:, 1] == LIVE_ALL).all()) and bool((first['b2.w2sm'][:, 1] < LIVE_ALL).all())
        before = {k: (v.data_ptr(), v.clone()) for k, v in first.items()}
        torch.manual_seed(99 + width)
        mutils.create(gen)                                                  # new modes: fresh codebooks
        second = check()
        assert any(not torch.equal(second[k], before[k][1]) for k in second)
        assert all(second[k].data_ptr() == before[k][0] for k in second)     # same shape: same address (captured graphs)
    finally:
        cfg.update(device='cuda')
        cfg.pop('classes_size', None)
