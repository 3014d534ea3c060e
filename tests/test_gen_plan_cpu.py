"""gen_plan.plan_generator (no GPU, no library) against what the commit before the plan existed decided.

tests/golden/gen_plan.json holds, per case, the plan's INPUTS (Linear / conv_a / head shapes, dtype, mode count, the
compacted pitch of every MultimodalController in the engine's order or null, the five flags) and the EXPECTED plan:
    routes[kind].blocks[i] = {a: [form, image], b: [form, image], x_compact, cap_h, y_ctrl, cap_y}, routes[kind].head,
    pm_enabled, buffers [[name, elements]], jobs [[weight, buffer, offset, elements, row_perm, kmajor, kmap, kcount, rmap]]
    (kmap / rmap: [controller, mode] or null), pm_controllers.

Where the expected values come from: the previous commit, not this code.  In a throw-away export of it (library built),
CPU models (cfg['device'] = 'cpu') were built per case from golden_util.procedural_state(seed 1234) -- codebooks then
overwritten where the case says so: rows with exactly k ones (a window that moves one channel per mode), or all ones for
"no pitch" -- with GE._MC / _GK / _PM / _PM_HEAD set per case.  ops.PrepBatch was replaced by a recorder and
GeneratorEngine._mode_maps by a stub returning zeros [modes, ops.cmap_stride(C)]; refresh_images() then gave the buffer
names and element counts (engine.img, without the fp32 'lin_bias') and every job's fields: the weight by data pointer,
the buffer / offset by storage, kmap / rmap as (controller, mode) by storage and storage offset of the stub tables and of
the _mode_perms cache.  The routes are the branch conditions of that commit's forward asked of its own methods
(_gk_enabled, _pm_enabled, _gk_block, _mc_block, _cap, _y_mc(i, pm and 'headm' in img), `name in engine.img`) for the
three kinds of pass; pm_controllers is its _pm_need() (empty where _pm_enabled() is false); caps are its _cap (null
where the compacted pass is off: the engine does not read them then).

Two input classes are routed differently on purpose; both are inputs on which the previous commit's pm pass FAILED:
  * "pm_refused" marks the one case of the first class (w64_active32): a compacted pitch below 64.  The previous commit
    gave the block per-mode images, and ops.conv_fused then refused the launch that reads them ("per-mode weight sets need
    the software-pipelined bf16 form (3x3 first segment of 64 .. 512 channels ...)").  The plan gives such a block no
    per-mode images: its pm route is the previous commit's gk route, the rest of the manifest is unchanged.
    test_the_marked_case_was_refused asks the kernel's own host plan (mcgen_conv_plan) for that refusal.
  * without a case: a gk-capable block whose mc_2 has NO pitch in front of a block whose pitches are all set.  The
    previous commit built that next block's per-mode images with a compacted shortcut while x arrived dense, and its pm
    pass then failed ops.conv_fused's image-size check; the plan gives such a block no per-mode images either, see
    test_per_mode_images_need_x_as_laid_out.
"""
import json
import os

from mcgen_amd import gen_plan as GP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'gen_plan.json')) as _f:
    CASES = json.load(_f)['cases']


def build(inputs, **over):
    d = dict(inputs, **over)
    return GP.plan_generator(tuple(d['lin']), [tuple(b) for b in d['blocks']], tuple(d['head']), d['dtype'] == 'bf16',
                             d['modes'], d['caps'], **d['flags'])


def as_json(plan):
    pair = lambda p: None if p is None else list(p)                          # noqa: E731
    routes = {}
    for kind in GP.KINDS:
        r = getattr(plan, kind)
        routes[kind] = {'blocks': [{'a': list(b.a), 'b': list(b.b), 'x_compact': b.x_compact, 'cap_h': b.cap_h,
                                    'y_ctrl': b.y_ctrl, 'cap_y': b.cap_y} for b in r.blocks], 'head': r.head}
    jobs = [[j.weight, j.buffer, j.offset, j.elems, j.row_perm, j.kmajor, pair(j.kmap), j.kcount, pair(j.rmap)] for j in plan.jobs]
    return {'routes': routes, 'pm_enabled': plan.pm_enabled, 'buffers': [list(b) for b in plan.buffers], 'jobs': jobs,
            'pm_controllers': list(plan.pm_controllers)}


def expected(case):
    """The previous commit's plan; for the "pm_refused" case without its per-mode images, the pm pass routed like gk."""
    want = case['plan']
    if case.get('pm_refused'):
        per_mode = lambda name: name.endswith(('.w2sm', '.w1m')) or name == 'headm'                     # noqa: E731
        want = dict(want, routes=dict(want['routes'], pm=want['routes']['gk']),
                    buffers=[b for b in want['buffers'] if not per_mode(b[0])], jobs=[j for j in want['jobs'] if not per_mode(j[1])])
        assert want['routes'] != case['plan']['routes'] and len(want['jobs']) < len(case['plan']['jobs'])
    return want


def test_plan_matches_the_previous_commit():
    assert len(CASES) >= 16 and [c['name'] for c in CASES if c.get('pm_refused')] == ['w64_active32']
    for c in CASES:
        got, want = as_json(build(c['inputs'])), expected(c)
        for kind in GP.KINDS:
            assert got['routes'][kind] == want['routes'][kind], (c['name'], kind)
        for k in ('pm_enabled', 'buffers', 'pm_controllers'):
            assert got[k] == want[k], (c['name'], k)
        assert len(got['jobs']) == len(want['jobs']), c['name']
        for i, (g, w) in enumerate(zip(got['jobs'], want['jobs'])):
            assert g == w, (c['name'], i, g, w)


def test_the_marked_case_was_refused():
    """The launch the previous commit's pm pass made first in the "pm_refused" case -- block 1's conv_b ++ shortcut at the
    smallest grouped batch (5 x 64 images): h compacted to the pitch as the 3x3 segment, dense x as the 1x1 segment, weight
    sets, permuted rows -- is refused by mcgen_conv_plan; the same launch at pitch 64 of the next case is taken."""
    import ctypes as C
    from mcgen_amd import _lib
    lib = _lib.load()
    by = {c['name']: c for c in CASES}
    for name, taken in (('w64_active32', False), ('w128_active64', True)):
        r = by[name]['plan']['routes']['pm']['blocks'][1]
        (ci, co, side), n = by[name]['inputs']['blocks'][1], 5 * 64
        assert r['b'][0] == 'pm' and not r['x_compact']
        p = _lib.Conv()
        p.nseg, p.N, p.H, p.W, p.Cout, p.Cout_w, p.Cy, p.alpha = 2, n, side, side, co, co, r['cap_y'] or co, 1.0
        p.w = p.y = p.bias = p.bias2 = p.wsel = 0x1000
        p.yperm, p.yperm_stride = (0x1000, co) if r['cap_y'] else (None, 0)
        p.wsel_stride = (r['cap_h'] // 32 * 9 + (ci + 31) // 32) * co * 32
        h, x = p.seg[0], p.seg[1]
        h.x = h.scale = h.shift = x.x = x.code = 0x1000
        h.C, h.ksize, h.relu, h.group_n = r['cap_h'], 3, 1, 1
        x.C, x.ksize, x.ups = ci, 1, 1
        rc = lib.mcgen_conv_plan(C.byref(p), 1, C.byref(_lib.ConvPlan()))
        assert (rc == 0) == taken, (name, lib.mcgen_last_error().decode())
        assert taken or 'per-mode weight sets need' in lib.mcgen_last_error().decode()


def test_issue_reference_values():
    """The two route tables read from the previous commit's own methods before the plan was written."""
    by = {c['name']: c for c in CASES}
    p = build(by['cifar10']['inputs'])
    assert by['cifar10']['inputs']['caps'] == [160] * 7 and p.pm_enabled
    assert [r.cap_h for r in p.gk.blocks] == [None, 160, 160] and [r.y_ctrl for r in p.gk.blocks] == [None, 4, None]
    assert [r.y_ctrl for r in p.pm.blocks] == [None, 4, 6] and p.pm.head == 'headm'
    p = build(by['coil100']['inputs'])
    assert by['coil100']['inputs']['caps'] == [288, 160, 160, 96, 96, None, None] and not p.pm_enabled
    assert all(r.y_ctrl is None and not r.x_compact for r in p.pm.blocks) and p.pm == p.gk


def test_cases_cover_every_form():
    a, b, heads, kinds_differ = set(), set(), set(), 0
    for c in CASES:
        p = build(c['inputs'])
        for kind in GP.KINDS:
            r = getattr(p, kind)
            a |= {x.a.form for x in r.blocks}
            b |= {x.b.form for x in r.blocks}
            heads.add(r.head)
            # every image a launch names exists, and compacted operands come with their pitches
            names = {n for n, _ in p.buffers}
            assert {l.image for x in r.blocks for l in (x.a, x.b)} | {r.head} <= names, c['name']
            assert r.layouts() == [0] + [GP.LAYOUT[l.form] for x in r.blocks for l in (x.a, x.b)] + [0]
        kinds_differ += p.plain != p.gk != p.pm
    assert a == {'dense', 'mc', 'gk', 'pm'} and b == {'dense', 'gk', 'pm'} and heads == {'head', 'headm'}
    assert kinds_differ >= 3
    names = {c['name'] for c in CASES}
    assert {'cifar10', 'coil100', 'modes16', 'modes17', 'w64_active32', 'w128_active64', 'w64_no_pitch', 'w32', 'cout288',
            'next_mc1_no_pitch', 'fp32', 'gk_off', 'pm_off', 'pm_head_off', 'mc_on'} <= names


def test_per_mode_images_need_x_as_laid_out():
    """Block 1 gk-capable without a pitch for its h: block 2's x arrives dense, so block 2 gets no per-mode images (they
    would hold a compacted shortcut) and takes the gk form in a pm pass; a zero pitch counts as none."""
    c = next(c for c in CASES if c['name'] == 'cifar10')
    for gone in (None, 0):
        p = build(c['inputs'], caps=[160, 160, 160, gone, 160, 160, 160])
        assert p.pm.blocks[1].b.form == 'dense' and not p.pm.blocks[2].x_compact
        assert (p.pm.blocks[2].a.form, p.pm.blocks[2].b.form) == ('dense', 'gk') and p.pm.head == 'head'
        assert not any(n.endswith(('m',)) for n, _ in p.buffers)


def test_image_sizes_match_the_library():
    from mcgen_amd import ops
    for cout, cin, ks in ((256, 256, 3), (3, 160, 3), (64, 32, 1), (288, 256, 3), (4096, 128, 1), (64, 100, 3)):
        assert GP.image_elems(cout, cin, ks) == ops.weight_image_elems(cout, cin, ks)
        assert GP.image_k_elems(cout, cin, ks) == ops.weight_image_k_elems(cout, cin, ks)
