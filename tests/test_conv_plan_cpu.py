"""The fused convolution's host decisions (no GPU): mcgen_conv_plan and the three older queries against values pinned from
the commit before the plan existed.

tests/golden/conv_plan.json holds descriptors AND expected answers.  A case is
    {"name", "dtype", "d": {mcgen_conv_t fields that differ from the defaults of `descriptor`}, "segs": [{mcgen_seg_t fields}],
     "rc", "err", "plan": {the twelve mcgen_conv_plan_t fields} or null, "queries": {"m_tiles", "tile": [rc, bm, bn], "form"},
     "queries_now": the same three, present only where this commit answers differently}
Pointer fields are 0 / 1 flags: a set pointer is the dummy address 0x1000.  The host code never dereferences a buffer and
makes no HIP call, so nothing here needs a GPU; mcgen_conv_fused is never called.

Where the expected values come from: the previous commit had no mcgen_conv_plan, so a throw-away copy of its csrc/ was
instrumented -- every launch_* of conv_fused.hip recorded (route, BM, BN, threads, mt, nt, lds, a_bytes, grouped) once `lds`
was final and returned before raise_lds, dispatch() recorded the pipe code, and the five `return mcgen_conv_<side kernel>()`
lines of mcgen_conv_fused recorded their route instead of launching.  That copy's mcgen_conv_fused (with a dummy `stats`
pointer where stats_mode is set, which its validate demands) gave rc / err / plan, and its unmodified mcgen_conv_m_tiles,
mcgen_conv_tile and mcgen_conv_form gave "queries".  plan.form is the old mcgen_conv_form answer, plan.m_tiles the old
mcgen_conv_m_tiles answer; bm / bn / pipe and the geometry are 0 for the five kernels in files of their own.

"queries_now" marks the only answers that moved: descriptors the previous commit's mcgen_conv_fused REFUSES, for which its
three hand-kept copies of the route chain disagreed with each other (mcgen_conv_m_tiles asked smap / px1 before it looked at
y_group, wsel or order; mcgen_conv_form had its own order).  The test checks that no accepted descriptor carries the mark.

One message of validate cannot come out of mcgen_conv_plan by construction: "stats_mode set without a stats buffer" (the
plan is asked before `stats` exists; mcgen_conv_fused still checks it).  Four more are unreachable through the shipped
policy and stay unpinned (as are the staging-plan "patch of ... pixels" checks, which none of these shapes trips; the 160 KB
check is pinned through the 256 x 256 mc tile): "no instantiation" (pick_tile only names table rows), the K-major "tiles ... must lie inside one
image" / "compacted output needs all channels in one tile" (mc_tile and validate guarantee both), and the wsel form of
"compacted output: the tile must hold all channels" (the pp tile is chosen from Cout_w).

The case list (see `coverage` checks below): every (BM, BN, pipe) row of f32_table and of the shipped bf16_table; both sides
of every pick_tile threshold (M = 16384, 32768, 65536, 131072 and one image less, at Cout_w = 16 .. 272, W = 16 / 32 / 64:
rows128 / rows256); grouped and plain dma3 (C = 352 / 384, and a tile whose three windows exceed 96 KB); cp at 64 and 128
pixels; pp at W = 16 / 32 on its three tiles; the pp_fits boundaries; the three mc and gk tiles and gk-pp; ycmap, yperm,
wsel, wsel + order, y_group; each side kernel with a near miss that falls through to the tiled route; the refusals.
"""
import ctypes as C
import json
import os

from mcgen_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'conv_plan.json')) as _f:
    CASES = json.load(_f)['cases']

DUMMY = 0x1000
SEG_PTRS = ('x', 'scale', 'shift', 'code', 'cmap')
SEG_INTS = ('C', 'ups', 'relu', 'ksize', 'group_n', 'cmap_stride', 'Cw')
PTRS = ('w', 'bias', 'y', 'res', 'ocode', 'gate_x', 'gscale', 'gshift', 'gmean', 'grstd', 'ycmap', 'bias2', 'wsel', 'order', 'yperm')
INTS = ('N', 'H', 'W', 'Cout', 'Cout_w', 'Cy', 'pool', 'tanh_out', 'stats_mode', 'w_layout', 'ycmap_stride', 'y_group',
        'wsel_stride', 'yperm_stride')
PLAN_FIELDS = ('route', 'form', 'bm', 'bn', 'pipe', 'm_tiles', 'grid_x', 'grid_y', 'threads', 'lds_bytes', 'a_bytes', 'grouped')
ROUTES = ('tiled', 'mc', 'gk', 'gk-pp', 'skinny', 'smap', 'px1', 'c8', 'head')


def descriptor(case):
    """mcgen_conv_t of a fixture case.  Defaults: x / w / y set, Cout_w = Cout rounded up to 16, Cy = Cout rounded up to 8,
    alpha 1, everything else zero; `stats` stays NULL (the plan must not need it)."""
    d = case['d']
    p = _lib.Conv()
    p.nseg = d.get('nseg', len(case['segs']))
    for i, s in enumerate(case['segs']):
        g = p.seg[i]
        for k in SEG_PTRS:
            setattr(g, k, DUMMY if s.get(k, 1 if k == 'x' else 0) else None)
        for k in SEG_INTS:
            setattr(g, k, s.get(k, 0))
    for k in PTRS:
        setattr(p, k, DUMMY if d.get(k, 1 if k in ('w', 'y') else 0) else None)
    cout = d.get('Cout', 0)
    for k in INTS:
        setattr(p, k, d.get(k, {'Cout_w': (cout + 15) // 16 * 16, 'Cy': (cout + 7) // 8 * 8}.get(k, 0)))
    p.alpha = 1.0
    return p


def queries(lib, p, dtype):
    bm, bn = C.c_int(-1), C.c_int(-1)
    rc = lib.mcgen_conv_tile(C.byref(p), dtype, C.byref(bm), C.byref(bn))
    return {'m_tiles': lib.mcgen_conv_m_tiles(C.byref(p), dtype), 'tile': [rc, bm.value, bn.value] if rc == 0 else [rc, -1, -1],
            'form': lib.mcgen_conv_form(C.byref(p), dtype)}


def test_plan_and_queries_match_the_previous_commit():
    lib = _lib.load()
    assert 200 <= len(CASES) <= 600
    for c in CASES:
        p, dtype = descriptor(c), c['dtype']
        out = _lib.ConvPlan()
        rc = lib.mcgen_conv_plan(C.byref(p) if not c['d'].get('null_p') else None, dtype, C.byref(out))
        assert (rc != 0) == (c['rc'] != 0), (c['name'], rc, lib.mcgen_last_error())
        if rc:
            assert lib.mcgen_last_error().decode() == c['err'], c['name']
        else:
            got = {k: getattr(out, k) for k in PLAN_FIELDS}
            assert got == c['plan'], (c['name'], got, c['plan'])
        if 'queries_now' in c:
            assert c['rc'] != 0, f"{c['name']}: a query may only change for a descriptor the previous commit refuses"
        if not c['d'].get('null_p'):
            assert queries(lib, p, dtype) == c.get('queries_now', c['queries']), c['name']
        # the plan reads no `stats`: the same answer with the buffer set
        if c['d'].get('stats_mode') and not rc:
            p.stats = DUMMY
            out2 = _lib.ConvPlan()
            assert lib.mcgen_conv_plan(C.byref(p), dtype, C.byref(out2)) == 0
            assert bytes(out2) == bytes(out), c['name']


def test_null_arguments():
    lib = _lib.load()
    out = _lib.ConvPlan()
    assert lib.mcgen_conv_plan(None, _lib.BF16, C.byref(out)) != 0
    assert lib.mcgen_last_error().decode() == 'conv_fused: nseg must be 1 or 2'
    assert lib.mcgen_conv_plan(C.byref(_lib.Conv()), _lib.BF16, None) != 0
    assert lib.mcgen_conv_m_tiles(None, _lib.BF16) == 0 and lib.mcgen_conv_form(None, _lib.BF16) == 0
    bm = C.c_int()
    assert lib.mcgen_conv_tile(None, _lib.BF16, C.byref(bm), C.byref(bm)) != 0
    assert lib.mcgen_last_error().decode() == 'conv_tile: null pointer'


# ---- the fixture covers what it has to --------------------------------------------------------------------------------
F32_ROWS = {(128, 16, 0), (64, 64, 0), (128, 128, 0)}
BF16_ROWS = {(256, 256, 5), (128, 256, 5), (128, 128, 5), (64, 128, 5), (64, 64, 11), (256, 16, 5), (64, 16, 12), (128, 16, 12),
             (256, 256, 20), (256, 128, 20), (128, 256, 20), (128, 64, 5)}
MESSAGES = [     # every reachable refusal of validate, the K-major checks and the route checks (prefix up to the first %)
    'conv_fused: nseg must be 1 or 2', 'conv_fused: H and W must be powers of two', 'conv_fused: W up to 64 supported',
    'conv_fused: Cout_w must be Cout rounded up to 16', 'conv_fused: Cy must be a positive multiple of 8',
    'conv_fused: null weight image or output', 'conv_fused: segment 0: C must be a positive multiple of 8',
    'conv_fused: segment 1: ksize must be 1 or 3', 'conv_fused: upsampled segment needs H, W >= 2',
    'conv_fused: segment 0: group_n must divide N', 'conv_fused: pooling needs H, W >= 2', 'conv_fused: bad stats_mode',
    'conv_fused: stats_mode 2 needs gate_x, gmean, grstd', 'conv_fused: unknown weight layout 3',
    'conv_fused: per-mode weight sets (wsel / order) go with the chunked weight image', 'conv_fused: wsel needs wsel_stride',
    'conv_fused: permuted weight rows (yperm) come with wsel', 'conv_fused: a compacted output takes bias and statistics only',
    'conv_fused: yperm: bad pitch', 'conv_fused: compacted output: bad pitch', 'conv_fused: a compacted output needs all channels in one tile',
    'conv_fused: Cy must be >= Cout',
    'conv_fused: K-major (mode-compacted) launches are bf16', 'conv_fused: K-major launch: segment 0 has no compaction map',
    'conv_fused(mc): at most 2048 channels per segment', 'conv_fused(mc): at least 64 output channels',
    'conv_fused(mc): no tile of a 8x8 map lies inside one image', 'conv_fused(mc): tile 256x256 needs 174336 bytes of LDS',
    'conv_fused: K-major launches are bf16', 'conv_fused(gk): segment 0: bad channel counts',
    'conv_fused(gk): segment 0: compacted channels need the map that orders them', 'conv_fused(gk): segment 0: map stride too small',
    'conv_fused(gk): segment 0: the code of a compacted segment rides in its scale / shift rows',
    'conv_fused(gk): at least 64 output channels', 'conv_fused(gk): no tile of a 8x8 map lies inside one image',
    'conv_fused: the paired output layout (y_group) is built for the image head only',
    'conv_fused: a compaction map needs a K-major launch', 'conv_fused: per-mode weight sets need the software-pipelined bf16 form',
    'conv_fused: yperm: the 256x256 tile must hold exactly the 144 channels',
    'conv_fused: compacted output: the 64x64 tile must lie inside one image and hold all',
    'conv_fused: tile of 64 pixels too small for W=64', 'conv_fused: a tile of 4 images would straddle BatchNorm groups of 2 images',
    'conv_fused: unknown dtype 7',
]


def _ok(route=None, dtype=None):
    return [c for c in CASES if c['rc'] == 0 and (route is None or ROUTES[c['plan']['route']] == route) and (dtype is None or c['dtype'] == dtype)]


def test_fixture_covers_every_table_row_route_and_refusal():
    rows = lambda dt: {(c['plan']['bm'], c['plan']['bn'], c['plan']['pipe']) for c in _ok('tiled', dt)}
    assert rows(_lib.F32) == F32_ROWS and rows(_lib.BF16) == BF16_ROWS
    for route in ROUTES:
        assert _ok(route), route
    tiles = lambda route: {(c['plan']['bm'], c['plan']['bn']) for c in _ok(route)}
    assert tiles('mc') == tiles('gk') == {(256, 256), (128, 256), (128, 128)} and tiles('gk-pp') == {(256, 256)}
    assert {c['plan']['grouped'] for c in _ok('tiled')} == {0, 1}
    assert {c['d']['W'] for c in _ok('tiled') if c['plan']['pipe'] == 20} == {16, 32}
    # the whole-image kernel: a statistics row per image, with one and with two images per workgroup (conv_smap.hip: im_pick)
    assert all(c['plan']['m_tiles'] == c['d']['N'] for c in _ok('smap'))
    assert {c['d']['N'] % 2 == 0 and c['d']['N'] * (c['d']['Cout'] // 64) >= 512 for c in _ok('smap')} == {False, True}
    assert {c['d']['H'] for c in _ok('px1')} == {4, 8, 16}
    for flag in ('ycmap', 'yperm', 'wsel', 'order', 'y_group'):
        assert any(c['d'].get(flag) for c in _ok()), flag
    errs = [c['err'] for c in CASES if c['rc'] != 0]
    for m in MESSAGES:
        assert any(e.startswith(m) for e in errs), m
    assert any('queries_now' in c for c in CASES)
