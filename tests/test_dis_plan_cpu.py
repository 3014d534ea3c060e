"""dis_plan.plan_discriminator (no GPU) against what the commit before the plan existed built.

tests/golden/dis_plan.json holds names and integers only.  Per case the plan's INPUTS:
    blocks[i] = {conv1, conv2, shortcut: [layer, cout, cin, ksize] or null, pooled, ctrl_x, ctrl_h}, tail [layer, controller],
    d0_fuse, image_cin (CGAN's image channels, else null), one_bucket
and the EXPECTED plan:
    images [[name, elements]], fwd / bwd / dimg job lists [[layer, buffer, offset, elements, transpose, sigma, 1 / wscale]]
    (1 / wscale is 1 or 4: the average pool's quarter), bucket_cut, and for MCGAN uses [[controller or null, layer]].

Where the expected values come from: the previous commit, not this code.  In a throw-away export of it (library built),
CPU models (cfg['device'] = 'cpu', freshly initialised: only shapes matter) were built per case with the discriminator
widths of the case, gan_engine._D0_FUSE set per case and ops.PrepBatch replaced by a recorder that keeps its job list;
after engine._ensure_flat(), engine._build_preps() then gave engine.img (names and element counts) and the batches in
construction order: forward, backward, both (checked to be forward + backward), and for CGAN the `0.dimg` batch.  Every
job's weight was identified by layer (`w is sn[k].m.weight_orig`; CGAN's two column copies `_w_img` by the layer they
copy), its buffer by the storage of the engine.img entry it lies in, its offset by storage_offset().  `uses` is that
commit's _code_uses(), bucket_cut its bucket_cut().  The inputs were read off the same engines: _SNConv.idx / cout / cin /
ks of the layers its index arithmetic resolves (conv[0] / conv[3] / shortcut[0], conv[2] / conv[5] / shortcut[1],
`len(conv) == 7`; CGAN: its _block(i)), controllers by identity in engine._codes.mcs.

Cases: MCGAN at CIFAR-10 and COIL100 widths, at the small fixtures' ([16] * 4 CIFAR-10 layout, [8, 16, 32, 64] COIL100
layout), with two blocks and with a single residual block (bucket_cut 0), each with MCGEN_D0_FUSE on and off; CGAN at
CIFAR-10 widths and at the small CIFAR-10 / Omniglot fixtures'.
"""
import json
import os

from mcgen_amd import dis_plan as DP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, 'tests', 'golden', 'dis_plan.json')) as _f:
    CASES = json.load(_f)['cases']
BY = {c['name']: c for c in CASES}


def build(inputs):
    layer = lambda l: None if l is None else DP.Layer(*l)                    # noqa: E731
    blocks = [DP.BlockFacts(layer(b['conv1']), layer(b['conv2']), layer(b['shortcut']), bool(b['pooled']), b['ctrl_x'], b['ctrl_h'])
              for b in inputs['blocks']]
    return DP.plan_discriminator(blocks, tuple(inputs['tail']), bool(inputs['d0_fuse']), inputs['image_cin'],
                                 bool(inputs['one_bucket']))


def jobs_json(jobs):
    out = []
    for j in jobs:
        assert 1.0 / j.wscale in (1.0, 4.0)
        out.append([j.layer, j.buffer, j.offset, j.elems, int(j.transpose), j.sigma, int(1.0 / j.wscale)])
    return out


def test_plan_matches_the_previous_commit():
    names = {c['name'] for c in CASES}
    want_names = {'cifar10', 'coil100', 'mcgan_small', 'coil_small', 'two_blocks', 'single_block'}
    assert want_names | {n + '_d0_unfused' for n in want_names} | {'cgan_cifar10', 'cgan_small', 'cgan_omniglot_small'} <= names
    for c in CASES:
        p, want = build(c['inputs']), c['plan']
        assert len(p.buffers) == len(want['images']) and dict(p.buffers) == {k: v for k, v in want['images']}, c['name']
        for k in ('fwd', 'bwd', 'dimg'):
            got = jobs_json(getattr(p, k))
            assert len(got) == len(want[k]), (c['name'], k)
            for i, (g, w) in enumerate(zip(got, want[k])):
                assert g == w, (c['name'], k, i, g, w)
        assert p.bucket_cut == want['bucket_cut'], c['name']
        if 'uses' in want:
            assert [list(u) for u in p.uses] == want['uses'], c['name']


def test_block_records():
    """The records say what the engines' walks derived: layer indices, pooling and its alpha, controllers, image names."""
    for c in CASES:
        p, inp = build(c['inputs']), c['inputs']
        names = dict(p.buffers)
        assert len(p.blocks) == len(inp['blocks']) and list(p.tail) == inp['tail']
        for i, (b, f) in enumerate(zip(p.blocks, inp['blocks'])):
            assert (b.conv1, b.conv2) == (f['conv1'][0], f['conv2'][0])
            assert b.shortcut == (f['shortcut'][0] if f['shortcut'] else None)
            assert b.pooled == bool(f['pooled']) and b.alpha == (0.25 if f['pooled'] else 1.0)
            assert (b.ctrl_x, b.ctrl_h) == (f['ctrl_x'], f['ctrl_h'])
            assert b.fused == (b.shortcut is not None and (i > 0 or bool(inp['d0_fuse'])))
            assert b.c1 == f'{i}.c1' and b.c2 == (f'{i}.c2s' if b.fused else f'{i}.c2') and b.c2t == f'{i}.c2t'
            assert b.sc == ('0.sc' if i == 0 and not b.fused else None)
            assert (b.c1t, b.dimg) == ((None, '0.dimg') if i == 0 else (f'{i}.c1t', None))
            assert b.sct == (f'{i}.sct' if i > 0 and b.shortcut is not None else None)
            # every image a block names exists
            assert {n for n in (b.c1, b.c2, b.sc, b.c2t, b.c1t, b.sct, b.dimg) if n} <= set(names), (c['name'], i)
        assert {n for b in p.blocks for n in (b.c1, b.c2, b.sc, b.c2t, b.c1t, b.sct, b.dimg) if n} == set(names)


def test_issue_reference_values():
    p = build(BY['cifar10']['inputs'])
    assert [(b.pooled, b.shortcut is not None) for b in p.blocks] == [(True, True), (True, True), (False, False), (False, False)]
    assert p.bucket_cut == 2 and p.uses[-1] == (7, 10) and p.uses[:3] == ((None, 0), (None, 2), (0, 1))
    assert dict(p.buffers)['0.c2s'] == dict(p.buffers)['0.c2t'] + 4096 and not p.dimg
    assert build(BY['single_block']['inputs']).bucket_cut == 0
    assert [b.c2 for b in build(BY['cifar10_d0_unfused']['inputs']).blocks[:2]] == ['0.c2', '1.c2s']
    c = build(BY['cgan_cifar10']['inputs'])
    assert c.bucket_cut == 0 and [j.buffer for j in c.dimg] == ['0.dimg'] * 2 and all(j.buffer != '0.dimg' for j in c.bwd)
    assert all(u[0] is None for u in c.uses)


def test_first_block_is_checked():
    import pytest
    f = BY['mcgan_small']['inputs']
    bad = dict(f, blocks=[dict(f['blocks'][0], shortcut=None)] + f['blocks'][1:])
    with pytest.raises(ValueError):
        build(bad)


def test_image_sizes_match_the_library():
    from mcgen_amd import ops
    for c in CASES:
        layers = {l[0]: l for b in c['inputs']['blocks'] for l in (b['conv1'], b['conv2'], b['shortcut']) if l}
        p = build(c['inputs'])
        for j in p.fwd + p.bwd:
            _, cout, cin, ks = layers[j.layer]
            assert j.elems == ops.weight_image_elems(cout, cin, ks, j.transpose), (c['name'], j)
        for j in p.dimg:
            _, cout, _, ks = layers[j.layer]
            assert j.elems == ops.weight_image_elems(cout, c['inputs']['image_cin'], ks, True), (c['name'], j)
