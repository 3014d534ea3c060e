"""Pins tests/px_sample_ref.py (the float64 reference test_px_sample_kernels_gpu.py holds csrc/pixelcnn_sample.hip to)
without a GPU: the whole-map forward against the oracle on square maps and against the row / column schedule on
non-square ones, the conditional form against the reference's recorded eval logits, the bf16 rounding points, and the
draw cases' probe sets."""
import pytest
import torch

import golden_util as gu
import px_sample_ref as R
from test_pixelcnn_sample_cpu import schedule_forward


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.fixture(scope='module')
def mc_state():
    return R.state(R.build('mcpixelcnn', 16, 4, 32))


def _inputs(h, w, n=5):
    g = torch.Generator().manual_seed(h * 100 + w)
    return torch.randint(0, 32, (n, h, w), generator=g), torch.randint(0, 10, (n,), generator=g)


@pytest.mark.parametrize('h,w', [(8, 8), (5, 5)])
def test_forward64_matches_oracle_on_square_maps(mc_state, h, w):
    from oracle import mcpixelcnn_oracle as O
    codes, label = _inputs(h, w)
    ref = O.forward({k: v.clone() for k, v in mc_state.items()}, codes, label, 10, train=False)['logits']
    got = R.forward64(mc_state, codes, label, 10, False)
    assert got.dtype == torch.float64 and got.shape == (5, 32, h, w)
    err = _rel(got, ref)
    print(f'forward64 vs oracle {h}x{w}: {err:.3g}')
    assert err < 1e-6


@pytest.mark.parametrize('h,w', [(5, 7), (2, 33), (1, 1)])
def test_forward64_matches_schedule_on_non_square_maps(mc_state, h, w):
    codes, label = _inputs(h, w)
    ref = schedule_forward(mc_state, codes, label, 10)
    err = _rel(R.forward64(mc_state, codes, label, 10, False), ref)
    print(f'forward64 vs schedule {h}x{w}: {err:.3g}')
    assert err < 1e-6


def test_forward64_is_causal_on_a_non_square_map(mc_state):
    """The logits at (i, j) do not move when a code at or after (i, j) in raster order does."""
    codes, label = _inputs(3, 6, n=2)
    base = R.forward64(mc_state, codes, label, 10, False)
    for i, j in [(0, 0), (1, 4), (2, 5)]:
        other = codes.clone()
        other[:, i, j] = (other[:, i, j] + 7) % 32
        moved = (R.forward64(mc_state, other, label, 10, False) != base).any(1)          # [N, H, W]
        flat, at = moved.reshape(2, -1), i * 6 + j
        assert not bool(flat[:, :at + 1].any())
        assert (i, j) == (2, 5) or bool(flat[:, at + 1:].any())


def test_conditional_forward64_matches_recorded_eval_logits():
    """test_cpixelcnn_cpu.py states no eval forward of its own; the statement of record is the reference's eval logits in
    cpixelcnn_small.npz on its trained state, which fp32 arithmetic reproduces to 1e-5 of max."""
    from test_cpixelcnn_gpu import _final_state
    d = gu.load_npz('cpixelcnn_small.npz')
    codes, label = torch.from_numpy(d['codes']), torch.from_numpy(d['label'])
    got = R.forward64(_final_state(d), codes, label, 10, True)
    err = _rel(got, torch.from_numpy(d['logits_eval']))
    print(f'conditional forward64 vs recorded eval logits: {err:.3g}')
    assert err < 1e-5


def test_conditional_form_reduces_to_the_controller_form():
    """With zero label rows and all-one controller codes the two forms are the same network."""
    mc, cp = R.state(R.build('mcpixelcnn', 16, 4, 32)), R.state(R.build('cpixelcnn', 16, 4, 32))
    for k in mc:
        if 'codebook' in k:
            mc[k] = torch.ones_like(mc[k])
            continue
        ck = k.replace('.module.', '.').replace('output_conv.4.', 'output_conv.3.')
        cp[ck] = mc[k].clone()
    for k in cp:
        if 'class_cond_embedding' in k:
            cp[k] = torch.zeros_like(cp[k])
    codes, label = _inputs(4, 7)
    assert torch.equal(R.forward64(mc, codes, label, 10, False), R.forward64(cp, codes, label, 10, True))
    cp['layers.2.class_cond_embedding.weight'][int(label[0])] += 1.0
    a, b = R.forward64(mc, codes, label, 10, False), R.forward64(cp, codes, label, 10, True)
    same = label != label[0]
    assert torch.equal(a[same], b[same]) and not torch.equal(a[0], b[0])


def test_bf16_store_rounds_logits_and_stays_near_float64(mc_state):
    codes, label = _inputs(5, 7)
    exact = R.forward64(mc_state, codes, label, 10, False)
    stored = R.forward64(mc_state, codes, label, 10, False, store=torch.bfloat16)
    assert torch.equal(stored, stored.bfloat16().double())
    err = _rel(stored, exact)
    assert 1e-4 < err < 5e-2, err                     # rounded somewhere, and no more than bf16 storage explains


# ---- the draw -------------------------------------------------------------------------------------------------------------
def test_inverse_cdf64_rule():
    lg = torch.tensor([0.0, -150.0, 0.0, 0.0, -150.0])
    u = torch.tensor([0.0, 0.3, 1 / 3, 0.5, 0.99, 1.0])
    k, dist = R.inverse_cdf64(lg, u)
    # S = 3 with boundaries at 0, 1, 1, 2, 3, 3: a boundary belongs to the next code with mass, u = 1 to the last one
    assert k.tolist() == [0, 0, 2, 2, 3, 3]
    assert float(dist[0]) == 0.0 and abs(float(dist[1]) - (1 / 3 - 0.3)) < 1e-7 and float(dist[5]) == 0.0
    # a mass below the smallest fp32 denormal counts as none, one above it counts
    k, _ = R.inverse_cdf64(torch.tensor([-104.0, 0.0, -103.0]), torch.tensor([0.0, 1.0]))
    assert k.tolist() == [1, 2]


@pytest.mark.parametrize('name,kq', R.DRAW_CASES)
def test_probe_sets(name, kq):
    lg = R.case_logits(name, kq)
    u, probed = R.probes(lg)
    assert u.dtype == torch.float32 and u.numel() == 3 * len(probed) + 3
    assert u[-3:].tolist() == [0.0, float(torch.tensor(1 - 2.0 ** -24, dtype=torch.float32)), 1.0] and float(u[-2]) < 1.0
    k, dist = R.inverse_cdf64(lg, u)
    # the margin is derived, not measured: the kernel's fp32 running sum is off by at most (ceil(Kq / 64) + 6 + 3) * 2^-24
    # of S (the lane's own adds, the six scan steps, exp and the product u * S): 1.01e-6 at Kq = 512, a ninth of the margin
    assert (-(-kq // 64) + 6 + 3) * 2.0 ** -24 * 9 <= R.MARGIN
    assert float(dist[:-3].min()) >= R.MARGIN, float(dist[:-3].min())
    assert k[:-3].tolist() == [c for c in probed for _ in range(3)]
    e, _ = R._cdf(lg[None])
    live = (e[0] > 0).nonzero().flatten().tolist()
    assert int(k[-3]) == live[0] and int(k[-1]) == live[-1]
    if name in ('flat', 'sparse'):
        assert probed == live
    if name == 'sparse':
        assert live == [3, kq - 5]
    if name == 'shifted':
        assert probed == R.shifted_peaks(kq) and len(live) == kq and int(k[-2]) == probed[-1]
    if name == 'gauss':
        print(f'gauss {kq}: {len(probed)} of {kq} codes probed')
        assert len(probed) >= 0.85 * kq
    print(f'{name} {kq}: {u.numel()} probes')
