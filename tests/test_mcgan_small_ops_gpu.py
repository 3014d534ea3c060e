"""The MCGAN kernels of csrc/small_ops.hip one at a time: spectral-norm power iteration (four-kernel, rounds and fused
forms), the spectral-norm gradient fix, the fused discriminator update (fix of both halves + Adam), Adam, the BatchNorm
statistics and backward, and column sums.  Shapes are the CIFAR-10 and COIL100 discriminator / generator sizes and the
size thresholds at which each kernel's unrolled or multi-pass loop starts.  test_mcgan_tail_code_ops_gpu.py does the same
for the discriminator tail, the hinge losses, tanh backward, the codes, the compaction maps and the layout kernels; the two
files together cover every kernel of small_ops.hip except the weight-image builders, which test_weight_image_gpu.py covers.

Every reference is float64 on the CPU (tests/small_ops_ref.py, itself checked against torch in
test_small_ops_ref_cpu.py), computed from exactly the fp32 values the kernel read.  Each bound is derived from the output
dtype, the accumulation length and the magnitudes of the terms:

- u = 2^-24 is the fp32 unit roundoff; a correctly rounded fp32 operation has relative error <= u.  A chain of n fp32
  additions or fmas, in any order and any grouping, has error at most n * u * (sum of the magnitudes of its terms), the
  gamma_n bound.  The kernels keep a fixed order of additions (sn_c1_kernel's comments say why); the bounds hold for any
  order, so they allow that order without demanding another.
- fp64 accumulation (BatchNorm, colsum stage 2) has unit roundoff 2^-53 and the same gamma_n bound.
- Where a bound is "doubled", the factor 2 covers second-order terms, device sqrt / division within 1 ulp (<= 2u), and
  the few extra roundings a count leaves out.

Buffers a kernel writes only in part start as NaN where it must not write, and must still be NaN afterwards.  Every
layer in a packed table is followed by a NaN gap, in the weights, the u / v state, the gradients and Adam's p, m, v, so a
read past a layer's end turns into a NaN in its result."""
import types
import zlib

import pytest
import torch

import golden_util as gu
import small_ops_ref as R
from mcgen_amd._lib import CONSTANTS

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
U16 = 2.0 ** -8
U64 = 2.0 ** -53
NAN = float('nan')
BN_FIN_MAX = CONSTANTS['MCGEN_BN_FIN_MAX']      # mcgen_bn_finalize_batch: layers per launch
BN_RUN_MAX = CONSTANTS['MCGEN_BN_RUN_MAX']      # mcgen_bn_running_batch: layers per launch (more run as several launches)
# thresholds that live only in csrc/small_ops.hip
SN_RS = 32              # sn_k1_wtu / sn_k3_wv / sn_c3_kernel: row slices per layer
SN_CS = 32              # sn_c1_kernel: column slices per layer; each slice walks its columns 64 at a time
SNC1_UNROLL_ROWS = 60   # sn_c1_kernel: the 16-load row loop runs while i + 60 < rows
SNC3_UNROLL_COLS = 704  # sn_c3_kernel: the 12-load column loop runs while j + 64 * 11 < cols
SNC1_MAX_ROWS = 1024    # sn_c1_kernel: u lives in su[1024] (mcgen_sn_power_iter_rounds refuses more)
SN_MAX_COLS = 15360     # sn_power_iter_impl: sn_k2_v keeps v in 60 KiB of LDS
SNF_LDS = 64 * 1024     # mcgen_sn_power_iter_fused: (max_cols + 2 max_rows + 32) floats of LDS at most
SNF_CHUNKS = 32         # sn_grad_dot(2)_kernel / sn_grad_apply(2)_kernel / sn_fix_pair_adam_kernel: dot partials per layer
SNF_BLOCK = 256         # sn_grad_dot2_kernel: threads per block; its 16-pair loop runs when a chunk exceeds 15 * 256
SNA_CHUNKS = 512        # sn_fix_pair_adam_kernel: blocks per layer (MCGEN_SNA_CHUNKS)
SNA_MIN = 1024          # sn_fix_pair_adam_kernel: elements per block at least
ADAM_GRID_CAP = 2048    # mcgen_adam: grid_for(n, 256, 2048); the 4-element loop runs when n > 3 * 2048 * 256
GRID_CAP = 4096         # grid_for's default cap (mcgen_bn_bwd_apply): its loop wraps when pixels * C / 8 > 4096 * 256
RED_SLOTS = 64          # reduce_partials: row slots per block (the slot loop takes a second trip above 64 rows)
RED_CPB = 16            # reduce_partials: channels per block
COLSUM_BLOCKS = 256     # mcgen_colsum: stage-1 blocks at most; colsum_stage2 adds them eight at a time


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % 100003


def _ops():
    from mcgen_amd import ops
    return ops


def _err():
    from mcgen_amd._lib import McgenError
    return McgenError


def _assert_within(got, ref, tol, what):
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        tol = tol.expand_as(ref) if torch.is_tensor(tol) else torch.full_like(ref, tol)
        raise AssertionError(f'{what}: {int(bad.sum())} of {err.numel()} outside the bound; first at flat index {i}: '
                             f'got {float(got.flatten()[i])}, ref {float(ref.flatten()[i])}, tol {float(tol.flatten()[i])}')


def _assert_nan_outside(flat, spans, what):
    """Every entry of `flat` outside the (offset, length) spans is still NaN."""
    keep = torch.ones(flat.numel(), dtype=torch.bool)
    for o, n in spans:
        keep[o:o + n] = False
    rest = flat.detach().cpu()[keep]
    assert torch.isnan(rest).all(), f'{what}: {int((~torch.isnan(rest)).sum())} entries outside the layers were written'


def _pack(tensors):
    """Offsets as gan_engine.FlatState lays them out (16-byte aligned, in order), with a NaN gap of 4 floats at least after
    every tensor -> (flat fp32 CPU tensor, offsets)."""
    offs, total = [], 0
    for t in tensors:
        offs.append(total)
        total += (t.numel() + 4 + 3) // 4 * 4
    flat = torch.full((total,), NAN)
    for t, o in zip(tensors, offs):
        flat[o:o + t.numel()] = t.reshape(-1)
    return flat, offs


def _unit(n, gen):
    return R.normalize(torch.randn(n, generator=gen, dtype=torch.float64)).float()


def _sn_table(ws, gen, plain=()):
    """Pack fp32 weights [rows, cols] (then plain parameters of the given sizes) as DiscriminatorEngine._ensure_flat does:
    SN layers first, then plain entries (rows = 0).  u, v start as random unit vectors."""
    us = [_unit(w.shape[0], gen) for w in ws]
    vs = [_unit(w.shape[1], gen) for w in ws]
    pl = [torch.randn(n, generator=gen) for n in plain]
    w_flat, w_offs = _pack(list(ws) + pl)
    uv = [t for pair in zip(us, vs) for t in pair]
    uv_flat, uv_offs = _pack(uv)
    layers = [(w_offs[i], uv_offs[2 * i], uv_offs[2 * i + 1], w.shape[0], w.shape[1]) for i, w in enumerate(ws)]
    layers += [(w_offs[len(ws) + k], 0, 0, 0, n) for k, n in enumerate(plain)]
    ops = _ops()
    return types.SimpleNamespace(
        ws=list(ws), us=us, vs=vs, plain=pl, w_flat=w_flat, uv_flat=uv_flat, layers=layers, n=len(ws),
        w=w_flat.cuda(), uv=uv_flat.cuda(), ld=ops.sn_layers_tensor(layers, 'cuda'),
        max_rows=max(w.shape[0] for w in ws), max_cols=max(w.shape[1] for w in ws))


def _seg(flat, off, n):
    return flat.detach().cpu()[off:off + n]


def _uv_spans(T):
    return [s for (_, uo, vo, r, c) in T.layers[:T.n] for s in ((uo, r), (vo, c))]


def _uv_of(T, flat, i):
    _, uo, vo, r, c = T.layers[i]
    return _seg(flat, uo, r), _seg(flat, vo, c)


def _sn_weights(d_hidden, num_mode, cifar):
    sh = gu.mcgan_shapes([64] * 4, d_hidden, num_mode, cifar_layout=cifar)
    return [(s[0], int(torch.tensor(s[1:]).prod())) for k, s in sh.items()
            if k.startswith('discriminator.') and k.endswith('weight_orig')]


CIFAR_D = _sn_weights([128] * 4, 10, True)                       # up to 128 x 1152, the 1 x 128 head
COIL_D = _sn_weights([64, 128, 256, 512], 100, False)            # up to 512 x 4608, the 1 x 512 head
THRESH_ROWS = [1, SNC1_UNROLL_ROWS, SNC1_UNROLL_ROWS + 1, 64, 65, SNC1_MAX_ROWS]
THRESH_COLS = [2, 31, SN_CS, SNC3_UNROLL_COLS, SNC3_UNROLL_COLS + 1, 2048, 2049, 4608]
WIDEST = {'four': (SNC1_MAX_ROWS, SN_MAX_COLS), 'rounds': (SNC1_MAX_ROWS, SN_MAX_COLS),
          'fused': (512, SNF_LDS // 4 - 2 * 512 - 32)}              # fused: exactly 64 KiB of LDS


def _shapes(table, form):
    if table == 'cifar':
        return CIFAR_D
    if table == 'coil':
        return COIL_D
    if table == 'thresholds':
        return [(r, c) for r in THRESH_ROWS for c in THRESH_COLS]
    if table == 'mixed':
        return [(1, 2), (SNC1_MAX_ROWS, 4608), (3, 5)]
    return [WIDEST[form], (2, 3)]


def _weights(shapes, gen, scale=0.05):
    return [torch.randn(r, c, generator=gen) * scale for r, c in shapes]


# ---- 1. power iteration -------------------------------------------------------------------------------------------------
def _check_round(w, u_in, u_k, v_k, s_k, what):
    """One training-mode round from the kernel's own previous u.

    v against normalize(W^T u_in): each W^T u entry is a chain of <= rows + 8 fp32 fmas / additions (c1: four chains per
    wave, four waves combined pairwise; k1: 32 row slices added in order; fused: four chains), so with a = |W|^T |u_in|,
    |d vt_j| <= (rows + 8) u a_j and |d |vt|| <= (rows + 8) u |a|; the norm itself is a sum of cols squares plus the
    slice / wave reductions, sqrt and reciprocal: relative (cols + 8) u.  tol_v = 2 ((rows + 8) u (a_j + |v_j| |a|) / |vt|
    + (cols + 8) u |v_j|).

    u and sigma against one float64 step from the kernel's own v (what its W v read), so the two halves do not compound:
    with b = |W| |v_k|, |d t_i| <= (cols + 8) u b_i (c3 / k3 / fused: one chain per lane over the columns, then a 64-lane
    shuffle tree), and the norm of t adds relative (rows + 8) u.  tol_u = 2 ((cols + 8) u (b_i + |u_i| |b|) / |t| +
    (rows + 8) u |u_i|); tol_sigma = 2 ((cols + 8) u |b| + (rows + 8) u sigma)."""
    rows, cols = w.shape
    w64 = w.double()
    vt = w64.t() @ u_in.double()
    a = w64.abs().t() @ u_in.double().abs()
    nv = vt.norm()
    v64 = vt / nv
    _assert_within(v_k, v64, 2 * ((rows + 8) * U32 * (a + v64.abs() * a.norm()) / nv + (cols + 8) * U32 * v64.abs()),
                   f'{what}: v')
    vk = v_k.double()
    t = w64 @ vk
    b = w64.abs() @ vk.abs()
    st = t.norm()
    u64 = t / st
    _assert_within(u_k, u64, 2 * ((cols + 8) * U32 * (b + u64.abs() * b.norm()) / st + (rows + 8) * U32 * u64.abs()),
                   f'{what}: u')
    _assert_within(torch.tensor([float(s_k)]), st.view(1), 2 * ((cols + 8) * U32 * b.norm() + (rows + 8) * U32 * st),
                   f'{what}: sigma')


def _check_eval(w, u, v, s_k, what):
    """Evaluation mode: sigma = u . (W v), a chain of cols fmas per row then rows products added:
    |d sigma| <= 2 (rows + cols + 16) u |u|^T |W| |v|."""
    rows, cols = w.shape
    ref = R.sigma_eval(w, u, v)
    tol = 2 * (rows + cols + 16) * U32 * float(u.double().abs() @ (w.double().abs() @ v.double().abs()))
    _assert_within(torch.tensor([float(s_k)]), torch.tensor([ref], dtype=torch.float64), tol, f'{what}: eval sigma')


def _run_form(T, form, rounds):
    """-> (sigma [rounds(+1), n] on the CPU, [snapshot per round] as flat CPU tensors); T.uv is updated in place."""
    ops = _ops()
    if form == 'four':
        sig, snaps = [], []
        for _ in range(rounds):
            s = torch.full((T.n,), NAN, device='cuda')
            snap = torch.full_like(T.uv, NAN)
            ops.sn_power_iter(T.w, T.uv, T.ld, T.n, True, s, T.max_rows, T.max_cols, snap=snap)
            torch.cuda.synchronize()
            _assert_nan_outside(snap, _uv_spans(T), 'sn_power_iter_snap: snapshot gaps')
            sig.append(s.cpu()); snaps.append(snap.cpu())
        return torch.stack(sig), snaps
    if form == 'four_nosnap':
        s = torch.full((T.n,), NAN, device='cuda')
        ops.sn_power_iter(T.w, T.uv, T.ld, T.n, True, s, T.max_rows, T.max_cols)
        torch.cuda.synchronize()
        return s.cpu().view(1, -1), [T.uv.cpu()]
    if form == 'rounds':
        sig, snap = ops.sn_power_iter_rounds(T.w, T.uv, T.ld, T.n, rounds, T.max_rows, T.max_cols)
    else:
        sig, snap = ops.sn_power_iter_fused(T.w, T.uv, T.ld, T.n, rounds, True, T.max_rows, T.max_cols)
    torch.cuda.synchronize()
    return sig.cpu(), [snap[r].cpu() for r in range(rounds)]


PI_FORMS = [('four_nosnap', 1), ('four', 1), ('four', 2), ('rounds', 1), ('rounds', 2), ('rounds', 3), ('fused', 1),
            ('fused', 2)]


@pytest.mark.parametrize('form,rounds', PI_FORMS)
@pytest.mark.parametrize('table', ['cifar', 'coil', 'thresholds', 'mixed', 'widest'])
def test_power_iteration(table, form, rounds):
    """Training-mode power iteration, every round checked by _check_round from the kernel's previous u (the initial u, then
    the snapshot of the round before).  'four' is mcgen_sn_power_iter (with a snapshot: mcgen_sn_power_iter_snap), 'rounds'
    mcgen_sn_power_iter_rounds (sn_c1 / sn_c3 per round, one sn_k4_u at the end), 'fused' mcgen_sn_power_iter_fused.

    Which case reaches which path: 'thresholds' crosses sn_c1's 16-load row loop (rows 60 -> 61, 64, 65, 1024), its
    second 64-column pass (cols 2049: 65 columns per slice) and sn_c3's 12-load column loop (cols 704 -> 705); 'coil' runs
    the 512 x 4608 layer through all of them; 'widest' is the widest layer each form accepts (1024 x 15360 for the four-kernel
    and rounds forms, 512 x 15328 = 64 KiB of LDS for the fused one); 'mixed' puts a 1 x 2 layer next to a 1024 x 4608 one.
    The state ends at the last snapshot; the extra sigma row of the rounds form (R >= 2) is sigma[R-2] / sigma[R-1] to
    within one fp32 division (2u, doubled); the u / v gaps stay NaN."""
    fam = form.split('_')[0]
    gen = torch.Generator().manual_seed(_seed(table, form, rounds))
    T = _sn_table(_weights(_shapes(table, fam), gen), gen)
    sig, snaps = _run_form(T, form, rounds)
    uv_end = T.uv.cpu()
    for r in range(rounds):
        for i, w in enumerate(T.ws):
            u_in = T.us[i] if r == 0 else _uv_of(T, snaps[r - 1], i)[0]
            u_k, v_k = _uv_of(T, snaps[r], i)
            _check_round(w, u_in, u_k, v_k, sig[r, i], f'{fam} round {r + 1}/{rounds}, layer {i} ({tuple(w.shape)})')
    for i in range(T.n):
        for a, b in zip(_uv_of(T, uv_end, i), _uv_of(T, snaps[-1], i)):
            assert torch.equal(a, b), f'layer {i}: the state is not the last snapshot'
    _assert_nan_outside(uv_end, _uv_spans(T), 'u / v state gaps')
    if form == 'rounds' and rounds >= 2:
        q = sig[rounds - 2].double() / sig[rounds - 1].double()
        _assert_within(sig[rounds], q, 4 * U32 * q.abs(), 'ratio row')


@pytest.mark.parametrize('form', ['four', 'fused'])
@pytest.mark.parametrize('table', ['cifar', 'coil', 'thresholds', 'widest'])
def test_power_iteration_eval(table, form):
    """Evaluation mode (mcgen_sn_power_iter with do_iter = 0, mcgen_sn_power_iter_fused with one round and do_iter = 0):
    u, v stay bit for bit, sigma = u . W v to the bound of _check_eval."""
    gen = torch.Generator().manual_seed(_seed(table, form, 'eval'))
    T = _sn_table(_weights(_shapes(table, form), gen), gen)
    before = T.uv.clone()
    if form == 'four':
        s = torch.full((T.n,), NAN, device='cuda')
        _ops().sn_power_iter(T.w, T.uv, T.ld, T.n, False, s, T.max_rows, T.max_cols)
    else:
        s, _ = _ops().sn_power_iter_fused(T.w, T.uv, T.ld, T.n, 1, False, T.max_rows, T.max_cols, snapshot=False)
        s = s[0]
    torch.cuda.synchronize()
    assert torch.equal(T.uv.isnan(), before.isnan()) and torch.equal(T.uv.nan_to_num(), before.nan_to_num())
    for i, w in enumerate(T.ws):
        _check_eval(w, T.us[i], T.vs[i], s[i].cpu(), f'{form} layer {i} ({tuple(w.shape)})')


@pytest.mark.parametrize('form,rounds', [('four', 1), ('rounds', 2), ('fused', 2)])
def test_power_iteration_exact_cases(form, rounds):
    """Closed forms.  rows = 1: sigma = |w|, u = +-1.  Rank one W = a b^T with small integer a, b (so W is exact in fp32):
    sigma = |a| |b|, u = +-a / |a|, v = +-b / |b|.  The bounds are _check_round's; sigma's adds |a| |b| times the bound on
    |v - b / |b||, since the float64 step from the kernel's v gives |a| |b . v|, not |a| |b|."""
    gen = torch.Generator().manual_seed(77)
    shapes = [(1, 2049), (1, 4608), (65, SNC3_UNROLL_COLS + 1), (SNC1_MAX_ROWS, 2049)]
    ab = []
    ws = []
    for r, c in shapes:
        a = torch.randint(1, 9, (r,), generator=gen).float() * (torch.randint(0, 2, (r,), generator=gen) * 2 - 1)
        b = torch.randint(1, 9, (c,), generator=gen).float() * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1)
        ab.append((a.double(), b.double()))
        ws.append(torch.outer(a, b) if r > 1 else b.view(1, -1))
    T = _sn_table(ws, gen)
    sig, snaps = _run_form(T, form, rounds)
    for r in range(rounds):
        for i, (w, (a, b)) in enumerate(zip(ws, ab)):
            rows, cols = w.shape
            u_k, v_k = _uv_of(T, snaps[r], i)
            if rows == 1:
                a = torch.ones(1, dtype=torch.float64)
            sv = torch.sign(float(v_k[0]) * b[0])
            su = torch.sign(float(u_k[0]) * a[0])
            vx, ux = sv * b / b.norm(), su * a / a.norm()
            u_in = T.us[i] if r == 0 else _uv_of(T, snaps[r - 1], i)[0]
            ain = w.double().abs().t() @ u_in.double().abs()
            nv = (w.double().t() @ u_in.double()).norm()
            tol_v = 2 * ((rows + 8) * U32 * (ain + vx.abs() * ain.norm()) / nv + (cols + 8) * U32 * vx.abs())
            _assert_within(v_k, vx, tol_v, f'{form} rank one {rows}x{cols}: v')
            bb = w.double().abs() @ v_k.double().abs()
            s64 = float(a.norm() * b.norm())
            _assert_within(u_k, ux, 2 * ((cols + 8) * U32 * (bb + ux.abs() * bb.norm()) / s64 + (rows + 8) * U32 * ux.abs()),
                           f'{form} rank one {rows}x{cols}: u')
            tol_s = 2 * ((cols + 8) * U32 * float(bb.norm()) + (rows + 8) * U32 * s64) + s64 * float(tol_v.norm())
            _assert_within(sig[r, i].view(1), torch.tensor([s64], dtype=torch.float64), tol_s, f'{form} rank one sigma')


def test_power_iteration_refusals():
    """Refused on the host before any launch: max_rows > 1024 in the rounds form (sn_c1's su[1024]), max_cols > 15360 in
    the four-kernel form (sn_k2_v's LDS), a layer beyond the fused form's 64 KiB LDS plan, and a rounds-form table whose
    widest layer has one column (its workspace plan needs max_cols + 32 + max_rows <= 32 max_cols + max_rows)."""
    gen = torch.Generator().manual_seed(5)
    ops, E = _ops(), _err()
    T = _sn_table(_weights([(SNC1_MAX_ROWS + 1, 8)], gen), gen)
    with pytest.raises(E, match='1024 rows'):
        ops.sn_power_iter_rounds(T.w, T.uv, T.ld, T.n, 2, T.max_rows, T.max_cols)
    T = _sn_table(_weights([(4, SN_MAX_COLS + 1)], gen), gen)
    with pytest.raises(E, match='15360'):
        ops.sn_power_iter(T.w, T.uv, T.ld, T.n, True, torch.zeros(1, device='cuda'), T.max_rows, T.max_cols)
    r, c = WIDEST['fused']
    T = _sn_table(_weights([(r, c + 1)], gen), gen)
    with pytest.raises(E, match='LDS plan'):
        ops.sn_power_iter_fused(T.w, T.uv, T.ld, T.n, 1, True, T.max_rows, T.max_cols)
    T = _sn_table(_weights([(5, 1), (3, 1)], gen), gen)
    with pytest.raises(E, match='workspace plan'):
        ops.sn_power_iter_rounds(T.w, T.uv, T.ld, T.n, 1, T.max_rows, T.max_cols)
    torch.cuda.synchronize()


# ---- 2. gradient fix ----------------------------------------------------------------------------------------------------
def _dot_depth(n):
    """Roundings one term of <G, W> goes through: a thread's chain over its share of a 1/32 chunk (<= chunk / 256 + 4),
    the four chains combined (2), the block reduction (6 shuffles + 4 waves) and the 32 chunk partials added in order."""
    return (n + SNF_CHUNKS - 1) // SNF_CHUNKS // SNF_BLOCK + 4 + 2 + 10 + SNF_CHUNKS


def _fix_ref(g, w, u, v, sigma):
    """(float64 fix, its bound).  o = (G - fl(fl(d / sigma) u_r) v_c) fl(1 / sigma) with d = <G, W> in fp32:
    |d d| <= k u sum |G W| (k = _dot_depth), the product X = d u_r v_c / sigma carries 3 roundings, the difference and the
    final product 3 more: |d o| <= 2 (3 u |G| + 6 u |X| + |d d| |u_r v_c| / sigma) / sigma (doubled)."""
    g64, w64, u64, v64 = (t.double() for t in (g, w, u, v))
    sigma = float(sigma)
    ref = R.grad_fix(g64, w64, u64, v64, sigma)
    d = float((g64 * w64).sum())
    dd = _dot_depth(w.numel()) * U32 * float((g64 * w64).abs().sum())
    uv = torch.outer(u64.abs(), v64.abs())
    tol = 2 * (3 * U32 * g64.abs() + 6 * U32 * abs(d) / sigma * uv + dd * uv / sigma) / sigma
    return ref, tol


FIX_SHAPES = [(128, 961), (127, 967), (61, SNC3_UNROLL_COLS + 1), (1, 31), (3, 3), (512, 4608)]
FIX_PLAIN = [1, 512, 513, 300001]


def _fix_table(table, gen):
    shapes = {'cifar': CIFAR_D, 'coil': COIL_D, 'sizes': FIX_SHAPES}[table]
    return _sn_table(_weights(shapes, gen), gen, plain=FIX_PLAIN)


def _grads(T, gen, corr=0.5):
    """A gradient per table entry, correlated with W (so <G, W> is large and a wrong pairing in the dot moves it), NaN in
    every gap."""
    gs = [corr * w + torch.randn(w.shape, generator=gen) * 0.05 for w in T.ws] + [torch.randn(p.shape, generator=gen) for p in T.plain]
    flat, _ = _pack(gs)
    return gs, flat


def _halves(T, gen):
    """A second u / v state and two sigmas, as the two forwards of a paired pass leave them."""
    us = [_unit(w.shape[0], gen) for w in T.ws]
    vs = [_unit(w.shape[1], gen) for w in T.ws]
    uv1, _ = _pack([t for pair in zip(us, vs) for t in pair])
    s0 = torch.rand(T.n, generator=gen) * 2 + 0.5
    s1 = torch.rand(T.n, generator=gen) * 2 + 0.5
    return us, vs, uv1, s0, s1


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('pair', [False, True])
@pytest.mark.parametrize('table', ['cifar', 'coil', 'sizes'])
def test_grad_fix(table, pair, accumulate):
    """mcgen_sn_grad_fix (pair = False) and mcgen_sn_grad_fix_pair against the float64 fix of _fix_ref per half; the pair's
    halves add with one more rounding each (+ 2u (|D| + |o_a| + |o_b|)).  'sizes' crosses sn_grad_dot2's 16-pair loop
    (128 x 961: chunks of 3844 > 15 * 256 elements; 127 x 967 stays just below), and has sizes not divisible by the 32
    chunks (61 x 705, 1 x 31, 3 x 3); 'coil' runs 2.4 M-element layers.  Plain entries (rows = 0; 1, 512, 513 and 300001
    elements) must come out exactly as fp32 A + B, (D + A) + B with accumulate; every gap of the destination stays NaN."""
    gen = torch.Generator().manual_seed(_seed(table, pair, accumulate))
    T = _fix_table(table, gen)
    ga, fa = _grads(T, gen)
    gb, fb = _grads(T, gen)
    us1, vs1, uv1, s0, s1 = _halves(T, gen)
    dst0 = torch.full_like(fa, NAN)
    dsts = [torch.randn(g.shape, generator=gen) for g in ga]
    if accumulate:
        for t, (o, *_) in zip(dsts, T.layers):
            dst0[o:o + t.numel()] = t.reshape(-1)
    dst = dst0.cuda()
    ops = _ops()
    if pair:
        ops.sn_grad_fix_pair(fa.cuda(), fb.cuda(), dst, T.w, T.uv, uv1.cuda(), T.ld, len(T.layers), s0.cuda(), s1.cuda(),
                             accumulate=accumulate)
    else:
        ops.sn_grad_fix(fa.cuda(), dst, T.w, T.uv, T.ld, len(T.layers), s0.cuda(), accumulate=accumulate)
    torch.cuda.synchronize()
    out = dst.cpu()
    for i, (o, _, _, rows, cols) in enumerate(T.layers):
        got = out[o:o + ga[i].numel()]
        base = dsts[i].reshape(-1) if accumulate else torch.zeros(ga[i].numel())
        if rows == 0:
            ref = base + ga[i] if accumulate else ga[i].clone()
            if pair:
                ref = ref + gb[i]
            assert torch.equal(got, ref.reshape(-1)), f'plain entry {i} ({cols}): not the fp32 sum'
            continue
        oa, ta = _fix_ref(ga[i], T.ws[i], T.us[i], T.vs[i], s0[i])
        tol = ta
        ref = oa
        if pair:
            ob, tb = _fix_ref(gb[i], T.ws[i], us1[i], vs1[i], s1[i])
            ref, tol = oa + ob, ta + tb + 2 * U32 * (oa.abs() + ob.abs())
        if accumulate:
            ref = ref + dsts[i].double()
            tol = tol + 2 * U32 * (dsts[i].double().abs() + ref.abs())
        _assert_within(got.view(rows, cols), ref, tol, f'{"pair" if pair else "single"} fix, layer {i} ({rows}x{cols})')
    _assert_nan_outside(out, [(o, r * c if r else c) for (o, _, _, r, c) in T.layers], 'destination gaps')


# ---- 3. fused discriminator update --------------------------------------------------------------------------------------
def _adam_tol(p, gi_ref, m, v, m2, v2, t, lr, b1, b2, eps, wd, dg):
    """Bound on (p', m', v') of one fp32 Adam update (adam_elem's arithmetic) whose gradient is known to within dg.
    g_i = fma(wd, p, g): |d g_i| <= dg + u |g_i|.  m' = fma(b1, m, (1 - b1) g_i): (1 - b1) dg_i + 3u ((1 - b1)|g_i| + b1 |m|).
    v' = fma(b2, v, (1 - b2) g_i g_i): (1 - b2)(2 |g_i| dg_i + dg_i^2) + 4u ((1 - b2) g_i^2 + b2 v).  sqrt(v'):
    min(dv' / (2 sqrt v'), sqrt dv') + 2u sqrt v'; den = sqrt(v') / bc2s + eps: that / bc2s + 3u sqrt(v') / bc2s + u den.
    q = step_size m' / den (step_size = lr / bc1 with bc1 rounded: 3u; the quotient and product: 2u):
    |dq| <= step_size dm' / den + |q| (dden / den + 5u); p' = p - q adds u |p'|.  All doubled."""
    bc1 = 1 - b1 ** t
    bc2s = (1 - b2 ** t) ** 0.5
    step = lr / bc1
    dgi = dg + (U32 * gi_ref.abs() if wd != 0 else 0.0)
    dm = (1 - b1) * dgi + 3 * U32 * ((1 - b1) * gi_ref.abs() + b1 * m.abs())
    dv = (1 - b2) * (2 * gi_ref.abs() * dgi + dgi * dgi) + 4 * U32 * ((1 - b2) * gi_ref * gi_ref + b2 * v.abs())
    sq = v2.clamp_min(0).sqrt()
    dsq = torch.minimum(dv / (2 * sq).clamp_min(1e-300), dv.sqrt()) + 2 * U32 * sq
    den = sq / bc2s + eps
    dden = dsq / bc2s + 3 * U32 * sq / bc2s + U32 * den
    q = step * m2 / den
    dq = step * dm / den + q.abs() * (dden / den + 5 * U32)
    p2 = p - q
    return 2 * (dq + U32 * p2.abs()), 2 * dm, 2 * dv


FUSED_SHAPES = [(1, 1), (1023, 1), (1024, 1), (1025, 1), (37, 27), (38, 27), (4, 255), (5, 255), (4, 256), (4, 257),
                (2048, 256), (2049, 256), (2057, 255), (2041, 257), (19419, 27), (524289, 1), (1, 4608), (512, 4608)]
FUSED_PLAIN = [1, 512, 513, 300001]
B1, B2, EPS = R.f32(0.5), R.f32(0.999), R.f32(1e-8)


@pytest.mark.parametrize('lr_form,wd', [('float', 0.0), ('dev', 0.125)])
@pytest.mark.parametrize('t', [1, 2, 1000, 1000000])
def test_fix_pair_adam(t, lr_form, wd):
    """mcgen_sn_fix_pair_adam against float64 Adam (small_ops_ref.adam) applied to fix(g0) + fix(g1), for two tables in the
    same step: the first advances the counter (advance_step), the second reads it.  Both must use t; the counter must read
    [t, 0] afterwards.  The gradient bound is test_grad_fix's pair bound; _adam_tol carries it through the update.

    Which case reaches which path: layers of 1, 1023, 1024, 1025 elements (one block, and the SNA_MIN boundary), 512 * 1024
    (2048 x 256: 1024 elements per block) and just above (2049 x 256, 2057 x 255, 2041 x 257, 19419 x 27, 524289 x 1: chunks
    above SNA_MIN), 512 x 4608; cols 1, 27, 255, 256, 257 and 4608 step the (row, column) pair with dr = 256 / cols,
    dc = 256 % cols below, at and above the block size; the 4-element loop runs in every block with 1024 or more elements.
    Plain entries of 1, 512, 513 and 300001 elements take Adam on the fp32 A + B.  t = 1, 2, 1000 and 10^6 pin adam_powi;
    lr comes as a float or as a device tensor; weight decay 0 or 0.125.  p, m, v keep NaN in every gap."""
    gen = torch.Generator().manual_seed(t + (7 if lr_form == 'dev' else 0))
    lr = R.f32(2e-4 * 7)
    ops = _ops()
    ws = _weights(FUSED_SHAPES, gen)
    split = 10
    tables = [_sn_table(ws[:split], gen, plain=FUSED_PLAIN[:2]), _sn_table(ws[split:], gen, plain=FUSED_PLAIN[2:])]
    step = torch.tensor([t - 1, 0], dtype=torch.int64, device='cuda')
    lr_arg = torch.tensor([lr], dtype=torch.float32, device='cuda') if lr_form == 'dev' else lr
    checks = []
    for k, T in enumerate(tables):
        ga, fa = _grads(T, gen)
        gb, fb = _grads(T, gen)
        us1, vs1, uv1, s0, s1 = _halves(T, gen)
        ms = [torch.randn(w.shape, generator=gen) * 1e-3 for w in T.ws] + [torch.randn(p.shape, generator=gen) * 1e-3 for p in T.plain]
        vs = [torch.rand(w.shape, generator=gen) * 1e-6 for w in T.ws] + [torch.rand(p.shape, generator=gen) * 1e-6 for p in T.plain]
        mf, _ = _pack(ms)
        vf, _ = _pack(vs)
        md, vd = mf.cuda(), vf.cuda()
        ops.sn_fix_pair_adam(fa.cuda(), fb.cuda(), T.w, md, vd, T.uv, uv1.cuda(), T.ld, len(T.layers), s0.cuda(), s1.cuda(),
                             step, lr_arg, (B1, B2), EPS, wd, advance_step=(k == 0))
        checks.append((T, ga, gb, us1, vs1, s0, s1, ms, vs, md, vd))
    torch.cuda.synchronize()
    assert step.tolist() == [t, 0], f'step counter {step.tolist()} after the update of step {t}'
    for T, ga, gb, us1, vs1, s0, s1, ms, vs, md, vd in checks:
        pf, mf, vf = T.w.cpu(), md.cpu(), vd.cpu()
        params = T.ws + T.plain
        spans = [(o, r * c if r else c) for (o, _, _, r, c) in T.layers]
        for i, (o, _, _, rows, cols) in enumerate(T.layers):
            n = params[i].numel()
            if rows == 0:
                g = (ga[i] + gb[i]).double()
                dg = torch.zeros_like(g)
            else:
                oa, ta = _fix_ref(ga[i], T.ws[i], T.us[i], T.vs[i], s0[i])
                ob, tb = _fix_ref(gb[i], T.ws[i], us1[i], vs1[i], s1[i])
                g, dg = (oa + ob).reshape(-1), (ta + tb + 2 * U32 * (oa.abs() + ob.abs())).reshape(-1)
            p0, m0, v0 = (x.reshape(-1).double() for x in (params[i], ms[i], vs[i]))
            p2, m2, v2 = R.adam(p0, g, m0, v0, t, lr, B1, B2, EPS, wd)
            gi = g + wd * p0
            tp, tm, tv = _adam_tol(p0, gi, m0, v0, m2, v2, t, lr, B1, B2, EPS, wd, dg)
            what = f't={t} layer {i} ({rows}x{cols})'
            _assert_within(mf[o:o + n], m2, tm, what + ': m')
            _assert_within(vf[o:o + n], v2, tv, what + ': v')
            _assert_within(pf[o:o + n], p2, tp, what + ': p')
        for name, f in (('p', pf), ('m', mf), ('v', vf)):
            _assert_nan_outside(f, spans, f'{name} gaps')


# ---- 4. Adam ------------------------------------------------------------------------------------------------------------
ADAM_N = [1, 3, 1000, 524288, 524289, 3 * ADAM_GRID_CAP * 256, 3 * ADAM_GRID_CAP * 256 + 1, 2097155, 4321290]


@pytest.mark.parametrize('seeded', [False, True])
@pytest.mark.parametrize('n', ADAM_N)
def test_adam(n, seeded):
    """mcgen_adam over three launches against float64 Adam step by step (each step from the kernel's own p, m, v), to the
    bound of _adam_tol with an exact gradient.  Unseeded: t = 1, 2, 3 from zero moments, lr as a float, no weight decay.
    Seeded: the counter starts at 10^6 - 1 with moments from earlier steps, lr as a device tensor, weight decay 0.01.
    One gradient in seven is exactly 0 and one in seven is 1e-12 (far below eps).  After every launch the counter and its
    ticket read [t, 0].  n = 1 .. 524288 runs one trip of the single-element loop, 524289 .. 1572864 several, 1572865 and
    above (2097155; 4321290, the CIFAR-10 generator) the 4-element loop plus the tail."""
    gen = torch.Generator().manual_seed(n % 9973 + seeded)
    ops = _ops()
    p = torch.randn(n, generator=gen) * 0.05
    m = torch.randn(n, generator=gen) * 1e-3 if seeded else torch.zeros(n)
    v = torch.rand(n, generator=gen) * 1e-6 if seeded else torch.zeros(n)
    t0 = 10 ** 6 - 1 if seeded else 0
    lr = R.f32(2e-4)
    wd = R.f32(0.01) if seeded else 0.0
    pd, md, vd = p.cuda(), m.cuda(), v.cuda()
    step = torch.tensor([t0, 0], dtype=torch.int64, device='cuda')
    lr_arg = torch.tensor([lr], dtype=torch.float32, device='cuda') if seeded else lr
    for k in range(3):
        g = torch.randn(n, generator=gen)
        g[::7] = 0.0
        g[1::7] = 1e-12
        p0, m0, v0 = pd.cpu().double(), md.cpu().double(), vd.cpu().double()
        ops.adam(pd, g.cuda(), md, vd, step, lr_arg, (B1, B2), EPS, wd)
        torch.cuda.synchronize()
        t = t0 + k + 1
        assert step.tolist() == [t, 0], f'after launch {k + 1}: step {step.tolist()}'
        p2, m2, v2 = R.adam(p0, g.double(), m0, v0, t, lr, B1, B2, EPS, wd)
        gi = g.double() + wd * p0
        tp, tm, tv = _adam_tol(p0, gi, m0, v0, m2, v2, t, lr, B1, B2, EPS, wd, torch.zeros_like(gi))
        _assert_within(md, m2, tm, f'n={n} t={t}: m')
        _assert_within(vd, v2, tv, f'n={n} t={t}: v')
        _assert_within(pd, p2, tp, f'n={n} t={t}: p')


# ---- 5. BatchNorm -------------------------------------------------------------------------------------------------------
def _bn_partials(tiles, fold, c, pitch, gen, const=False):
    """[tiles, 2, pitch] per-tile (sum, sum of squares) of 8 pixels per fold lane, NaN in the pad lanes [fold C, pitch):
    channel means around 1, every lane's own variance s2 / 8 - (s1 / 8)^2 between 0.25 and 0.75 of the channel's (so the
    pooled variance is positive).  const: channel 0 holds a constant 0.1 with its sum of squares nudged down by 2^-20
    relative, so s2 / count - mean^2 < 0 and the variance clamp must act."""
    mu = torch.randn(c, generator=gen).double() + 1.0
    var = torch.rand(c, generator=gen).double() + 0.5
    s1 = 8 * mu + (8 * var).sqrt() * torch.randn(tiles, fold, c, generator=gen, dtype=torch.float64)
    s2 = s1 * s1 / 8 + 8 * var * (0.25 + 0.5 * torch.rand(tiles, fold, c, generator=gen, dtype=torch.float64))
    s1, s2 = s1.float(), s2.float()
    if const:
        k = R.f32(0.1)
        s1[..., 0] = 8 * k
        s2[..., 0] = float(torch.tensor(8 * k * k, dtype=torch.float32)) * (1 - 2.0 ** -20)
    part = torch.full((tiles, 2, pitch), NAN)
    part[:, 0, :fold * c] = s1.reshape(tiles, fold * c)
    part[:, 1, :fold * c] = s2.reshape(tiles, fold * c)
    return part


def _bn_sums(part, groups, fold, c):
    """Per group: float64 (s1, s2, sum |s1|, sum |s2|, terms) over the group's tiles and fold lanes."""
    tiles = part.shape[0]
    p = part[:, :, :fold * c].double().reshape(groups, tiles // groups, 2, fold, c)
    s = p.sum((1, 3))
    a = p.abs().sum((1, 3))
    return s[:, 0], s[:, 1], a[:, 0], a[:, 1], tiles // groups * fold + RED_SLOTS


def _bn_ref_tol(part, groups, fold, c, count, gamma, beta, eps):
    """float64 statistics per group and their bounds.  The sums are fp64 chains over the tile rows plus the 64-slot combine
    (k terms): |d s| <= k 2^-53 sum |s|.  mean = s1 / count, var = s2 / count - mean^2 in fp64 (clamped at 0), each output
    rounded to fp32 once: mean u |mean|; rstd (fp64 sqrt and reciprocal, then fp32) u rstd + rstd dvar / (2 (var + eps));
    scale = gamma rstd: one more u; shift = beta - fl(mean) scale: 2u |mean scale| + u |shift| on top of the mean and scale
    errors; unbiased var: u |unb| + dvar count / (count - 1).  Doubled."""
    s1, s2, a1, a2, k = _bn_sums(part, groups, fold, c)
    st = R.bn_stats(s1, s2, count, gamma.double(), beta.double(), eps)
    dm = k * U64 * a1 / count + 4 * U64 * st['mean'].abs()
    dvar = k * U64 * a2 / count + 2 * st['mean'].abs() * dm + 4 * U64 * (s2.abs() / count + st['mean'] ** 2)
    tol = {'mean': U32 * st['mean'].abs() + dm}
    tol['rstd'] = U32 * st['rstd'] + st['rstd'] * dvar / (2 * (st['var'] + eps))
    tol['scale'] = gamma.double().abs() * tol['rstd'] + U32 * st['scale'].abs()
    tol['shift'] = (tol['mean'] * st['scale'].abs() + st['mean'].abs() * tol['scale'] + 2 * U32 * (st['mean'] * st['scale']).abs()
                    + U32 * st['shift'].abs())
    tol['unb'] = U32 * st['unb'].abs() + dvar * (count / (count - 1) if count > 1 else 1.0)
    return st, {k_: 2 * v_ for k_, v_ in tol.items()}


def _running_ref_tol(rm, rv, st, tol, momentum):
    """Running statistics after the groups' updates in order, each (1 - m) r + m x in fp32 (1 - m rounded: 4 roundings):
    |d r'| <= (1 - m) |d r| + m |d x| + 4u ((1 - m) |r| + m |x|), x being the fp32 mean / unbiased variance."""
    m = momentum
    out = []
    for r, key in ((rm.double(), 'mean'), (rv.double(), 'unb')):
        d = torch.zeros_like(r)
        for g in range(st[key].shape[0]):
            x = st[key][g]
            d = (1 - m) * d + m * tol[key][g] + 4 * U32 * ((1 - m) * r.abs() + m * x.abs())
            r = (1 - m) * r + m * x
        out += [r, 2 * d]
    return out


def _bn_params(c, gen):
    return (torch.randn(c, generator=gen) * 0.2 + 1), torch.randn(c, generator=gen) * 0.1


@pytest.mark.parametrize('c', [1, 16, 17, 256, 512])
@pytest.mark.parametrize('tpg', [1, 63, 64, 65, 1024])
def test_bn_finalize(tpg, c):
    """mcgen_bn_finalize_groups (ops.bn_finalize) against _bn_ref_tol for groups 1 and 5 (tiles = tpg x groups), fold 1 and
    3 with pitch = fold C + 5 (NaN pads), running statistics with momentum 0.1 (groups 1) and 0.3 (groups 5) updated in
    group order (_running_ref_tol).  Channel 0 is constant (the variance clamp) when C > 1.  reduce_partials' slot loop takes
    a second trip once tpg x fold > 64 (tpg 65, 1024, and 63 with fold 3); C = 17 leaves a partial 16-channel block."""
    ops = _ops()
    for groups, fold, mom in ((1, 1, 0.1), (5, 1, 0.3), (1, 3, 0.1), (5, 3, 0.3)):
        gen = torch.Generator().manual_seed(tpg * 1000 + c + groups * 7 + fold)
        tiles, pitch = tpg * groups, fold * c + 5
        part = _bn_partials(tiles, fold, c, pitch, gen, const=c > 1)
        gamma, beta = _bn_params(c, gen)
        rm, rv = torch.randn(c, generator=gen) * 0.1, torch.rand(c, generator=gen) + 0.5
        count = tpg * fold * 8
        rmd, rvd = rm.cuda(), rv.cuda()
        sc, sh, mean, rstd = ops.bn_finalize(part.cuda(), count, gamma.cuda(), beta.cuda(), rmd, rvd, momentum=R.f32(mom),
                                             eps=1e-5, fold=fold, groups=groups)
        torch.cuda.synchronize()
        st, tol = _bn_ref_tol(part, groups, fold, c, count, gamma, beta, R.f32(1e-5))
        what = f'groups={groups} fold={fold} tiles={tiles} C={c}'
        for name, got in (('scale', sc), ('shift', sh), ('mean', mean), ('rstd', rstd)):
            _assert_within(got.view(groups, c), st[name], tol[name], f'{what}: {name}')
        erm, trm, erv, trv = _running_ref_tol(rm, rv, st, tol, R.f32(mom))
        _assert_within(rmd, erm, trm, f'{what}: running mean')
        _assert_within(rvd, erv, trv, f'{what}: running var')


def test_bn_finalize_count_one_and_no_running_stats():
    """count = 1 (one pixel per channel: the unbiased variance is the biased one, here 0 after the clamp), momentum 0.75,
    and the same partials without running statistics."""
    ops = _ops()
    gen = torch.Generator().manual_seed(4)
    c = 20
    x = torch.randn(c, generator=gen)
    part = torch.full((1, 2, c + 3), NAN)
    part[0, 0, :c], part[0, 1, :c] = x, x * x
    gamma, beta = _bn_params(c, gen)
    rm, rv = torch.randn(c, generator=gen), torch.rand(c, generator=gen) + 0.5
    rmd, rvd = rm.cuda(), rv.cuda()
    sc, sh, mean, rstd = ops.bn_finalize(part.cuda(), 1, gamma.cuda(), beta.cuda(), rmd, rvd, momentum=0.75, eps=1e-5)
    sc2, sh2, mean2, rstd2 = ops.bn_finalize(part.cuda(), 1, gamma.cuda(), beta.cuda(), None, None, momentum=0.75, eps=1e-5)
    torch.cuda.synchronize()
    st, tol = _bn_ref_tol(part, 1, 1, c, 1, gamma, beta, R.f32(1e-5))
    for name, got, got2 in (('scale', sc, sc2), ('shift', sh, sh2), ('mean', mean, mean2), ('rstd', rstd, rstd2)):
        _assert_within(got.view(1, c), st[name], tol[name], f'count 1: {name}')
        assert torch.equal(got, got2)
    erm, trm, erv, trv = _running_ref_tol(rm, rv, st, tol, 0.75)
    _assert_within(rmd, erm, trm, 'count 1: running mean')
    _assert_within(rvd, erv, trv, 'count 1: running var')


@pytest.mark.parametrize('running', [False, True])
def test_bn_finalize_batch(running):
    """mcgen_bn_finalize_batch with MCGEN_BN_FIN_MAX jobs of different C (17, 256, 1, 40), tiles (65, 1, 200, 3) and pitch,
    every job against _bn_ref_tol; running statistics (momentum 0.2) on every job or on none."""
    ops = _ops()
    gen = torch.Generator().manual_seed(9 + running)
    specs = [(17, 65), (256, 1), (1, 200), (40, 3)][:BN_FIN_MAX]
    items, refs = [], []
    for c, tiles in specs:
        part = _bn_partials(tiles, 1, c, c + 3, gen, const=c > 1)
        gamma, beta = _bn_params(c, gen)
        rm, rv = torch.randn(c, generator=gen) * 0.1, torch.rand(c, generator=gen) + 0.5
        rmd, rvd = (rm.cuda(), rv.cuda()) if running else (None, None)
        items.append((part.cuda(), tiles * 8, gamma.cuda(), beta.cuda(), rmd, rvd, R.f32(0.2), R.f32(1e-5)))
        refs.append((part, c, tiles * 8, gamma, beta, rm, rv, rmd, rvd))
    outs = ops.bn_finalize_batch(items)
    torch.cuda.synchronize()
    for (part, c, count, gamma, beta, rm, rv, rmd, rvd), out in zip(refs, outs):
        st, tol = _bn_ref_tol(part, 1, 1, c, count, gamma, beta, R.f32(1e-5))
        for name, got in zip(('scale', 'shift', 'mean', 'rstd'), out):
            _assert_within(got.view(1, c), st[name], tol[name], f'batch job C={c}: {name}')
        if running:
            erm, trm, erv, trv = _running_ref_tol(rm, rv, st, tol, R.f32(0.2))
            _assert_within(rmd, erm, trm, f'batch job C={c}: running mean')
            _assert_within(rvd, erv, trv, f'batch job C={c}: running var')


def test_bn_finalize_par_and_running_batch():
    """The grouped generator pass's path: mcgen_bn_finalize_par for 30 layers of 5 statistics groups (C from 1 to 520, fold
    1 or 2), then ONE ops.bn_running_batch over all 30 (more than MCGEN_BN_RUN_MAX = 24: two launches), momentum 0.1 or 0.3.
    Scale / shift / mean / rstd / unbiased variance per group against _bn_ref_tol, the running statistics against
    _running_ref_tol (the groups' updates in order)."""
    ops = _ops()
    gen = torch.Generator().manual_seed(21)
    njobs = BN_RUN_MAX + 6
    groups = 5
    items, checks = [], []
    for j in range(njobs):
        c = [1, 16, 17, 256, 257, 300, 520][j % 7]
        fold = 1 + j % 2
        tpg = [1, 13, 65][j % 3]
        part = _bn_partials(tpg * groups, fold, c, fold * c + 3, gen, const=c > 1)
        gamma, beta = _bn_params(c, gen)
        rm, rv = torch.randn(c, generator=gen) * 0.1, torch.rand(c, generator=gen) + 0.5
        count = tpg * fold * 8
        sc, sh, mean, rstd, unb = ops.bn_finalize_par(part.cuda(), count, gamma.cuda(), beta.cuda(), eps=1e-5, fold=fold,
                                                      groups=groups)
        rmd, rvd = rm.cuda(), rv.cuda()
        mom = R.f32(0.1 if j % 2 else 0.3)
        items.append((rmd, rvd, mean, unb, mom))
        checks.append((part, fold, c, count, gamma, beta, rm, rv, rmd, rvd, mom, (sc, sh, mean, rstd, unb)))
    ops.bn_running_batch(items)
    torch.cuda.synchronize()
    for part, fold, c, count, gamma, beta, rm, rv, rmd, rvd, mom, outs in checks:
        st, tol = _bn_ref_tol(part, groups, fold, c, count, gamma, beta, R.f32(1e-5))
        what = f'par C={c} fold={fold} count={count}'
        for name, got in zip(('scale', 'shift', 'mean', 'rstd', 'unb'), outs):
            _assert_within(got, st[name], tol[name], f'{what}: {name}')
        erm, trm, erv, trv = _running_ref_tol(rm, rv, st, tol, mom)
        _assert_within(rmd, erm, trm, f'{what}: running mean')
        _assert_within(rvd, erv, trv, f'{what}: running var')


@pytest.mark.parametrize('c', [1, 17, 512])
def test_bn_eval_affine(c):
    """mcgen_bn_eval_affine: scale = gamma / sqrtf(rv + eps) (add, sqrt, divide: 5u), shift = beta - rm scale:
    |rm| dscale + 2u |rm scale| + u |shift|.  Doubled."""
    gen = torch.Generator().manual_seed(c)
    gamma, beta = _bn_params(c, gen)
    rm, rv = torch.randn(c, generator=gen), torch.rand(c, generator=gen) * 2
    rv[0] = 0.0
    sc, sh = _ops().bn_eval_affine(gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), eps=1e-5)
    torch.cuda.synchronize()
    esc, esh = R.bn_eval_affine(gamma, beta, rm, rv, R.f32(1e-5))
    tsc = 2 * 5 * U32 * esc.abs()
    _assert_within(sc, esc, tsc, 'eval scale')
    _assert_within(sh, esh, 2 * (rm.double().abs() * tsc + 2 * U32 * (rm.double() * esc).abs() + U32 * esh.abs()), 'eval shift')


BWD_CASES = [((2, 5, 5, 8), torch.float32, True, True, True), ((2, 5, 5, 8), torch.float32, False, False, False),
             ((2, 5, 5, 8), torch.bfloat16, True, False, True), ((2, 5, 5, 8), torch.bfloat16, False, True, False),
             ((2, 5, 5, 8), torch.float32, True, True, None),
             ((64, 32, 32, 256), torch.float32, True, True, True), ((64, 32, 32, 256), torch.bfloat16, False, False, False)]


@pytest.mark.parametrize('shape,dtype,add,accumulate,grads', BWD_CASES)
def test_bn_backward(shape, dtype, add, accumulate, grads):
    """ops.bn_backward: mcgen_bn_bwd_finalize (fp64 sums of [70, 2, C + 8] partials with NaN pads -> fp32 sums, dgamma /
    dbeta stored or accumulated, or None) and mcgen_bn_bwd_apply.  dx = scale (dz - s1 / n - xh s2 / n) with
    xh = (x - mean) rstd in fp32: with T1 = |dz|, T2 = |s1 / n|, T3 = |xh s2 / n|, |d dx| <= |scale| (2u T1 + 5u T2 + 8u T3)
    + u |dx| (+ u |dx + add|), doubled; a bf16 output adds 2^-8 |ref|.  64 x 32 x 32 x 256 gives pixels C / 8 = 2 M vectors
    of 8, twice 4096 x 256: the grid-stride loop wraps."""
    ops = _ops()
    gen = torch.Generator().manual_seed(shape[0] + shape[-1] + (dtype == torch.bfloat16) + 2 * add + 4 * accumulate)
    c = shape[-1]
    count = shape[0] * shape[1] * shape[2]
    tiles = 70
    part = torch.full((tiles, 2, c + 8), NAN)
    part[:, :, :c] = torch.randn(tiles, 2, c, generator=gen) * 4
    scale, mean = torch.randn(c, generator=gen), torch.randn(c, generator=gen) * 0.5
    rstd = torch.rand(c, generator=gen) + 0.5
    dz = torch.randn(shape, generator=gen).to(dtype)
    x = torch.randn(shape, generator=gen).to(dtype)
    addt = torch.randn(shape, generator=gen).to(dtype) if add else None
    dg0, db0 = torch.randn(c, generator=gen), torch.randn(c, generator=gen)
    dgd, dbd = (dg0.cuda(), db0.cuda()) if grads else (None, None)
    dx = ops.bn_backward(part.cuda(), dz.cuda(), x.cuda(), count, scale.cuda(), mean.cuda(), rstd.cuda(), dgd, dbd,
                         add=addt.cuda() if add else None, accumulate=accumulate)
    torch.cuda.synchronize()
    p64 = part[:, :, :c].double()
    s64 = p64.sum(0)
    a64 = p64.abs().sum(0)
    ds = (tiles + RED_SLOTS) * U64 * a64
    s32 = s64.float().double()                              # the sums the apply kernel reads, rounded to fp32 once
    inv = R.f32(1.0 / count)
    if grads:
        for got, base, k, name in ((dgd, dg0, 1, 'dgamma'), (dbd, db0, 0, 'dbeta')):
            ref = s64[k] + (base.double() if accumulate else 0)
            tol = 2 * (ds[k] + U32 * s64[k].abs() + (U32 * ref.abs() if accumulate else 0))
            _assert_within(got, ref, tol, name)
    ref = R.bn_backward(dz.reshape(-1, c), x.reshape(-1, c), 1.0 / inv, scale, mean, rstd, s32[0], s32[1],
                        add=addt.reshape(-1, c) if add else None)
    xh = (x.reshape(-1, c).double() - mean.double()) * rstd.double()
    t1, t2, t3 = dz.reshape(-1, c).double().abs(), (s32[0] * inv).abs(), (xh * s32[1] * inv).abs()
    core = scale.double() * (dz.reshape(-1, c).double() - s32[0] * inv - xh * s32[1] * inv)
    t32 = scale.double().abs() * (2 * U32 * t1 + 5 * U32 * t2 + 8 * U32 * t3) + U32 * core.abs()
    if add:
        t32 = t32 + U32 * ref.abs()
    t32 = 2 * t32
    tol = t32 if dtype == torch.float32 else t32 + U16 * (ref.abs() + t32)
    _assert_within(dx.reshape(-1, c), ref, tol, f'dx {dtype} {shape}')


# ---- 6. column sums -----------------------------------------------------------------------------------------------------
def _colsum_tol(x, c, alpha, rows, base=None):
    """Stage 1: a block's fp32 chain over rpb = ceil(rows / min(rows, 256)) rows; stage 2 adds the blocks in fp64 and rounds
    once; alpha * s rounds once more; accumulate adds one rounding of the sum:
    |d out| <= 2 (|alpha| (rpb u + 256 2^-53) sum |x| + 2u |alpha s| (+ u |out|))."""
    blocks = min(rows, COLSUM_BLOCKS)
    rpb = (rows + blocks - 1) // blocks
    xs = x.double().reshape(-1, x.shape[-1])[:, :c]
    s = alpha * xs.sum(0)
    t = abs(alpha) * (rpb * U32 + COLSUM_BLOCKS * U64) * xs.abs().sum(0) + 2 * U32 * s.abs()
    if base is not None:
        t = t + U32 * (s + base.double()).abs()
    return 2 * t


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('c', [1, 3, 130])
@pytest.mark.parametrize('rows', [1, 255, 256, 257, 131075])
def test_colsum(rows, c, dtype):
    """mcgen_colsum over [rows, C + 6] with NaN pads and a positive mean (so a dropped block shows), alpha = 0.75: stored
    into a NaN buffer one longer than C (the extra entry stays NaN), then accumulated onto random values.  rows >= 8 runs
    colsum_stage2's 8-load loop (255: 31 trips and a 7-block tail), 131075 rows give stage 1 blocks of 513 rows."""
    ops = _ops()
    gen = torch.Generator().manual_seed(rows + c)
    pitch = c + 6
    x = torch.full((rows, pitch), NAN)
    x[:, :c] = torch.randn(rows, c, generator=gen) + 1.0
    x = x.to(dtype)
    xd = x.cuda()
    out = torch.full((c + 1,), NAN, device='cuda')
    ops.colsum(xd, c, out[:c], alpha=0.75)
    torch.cuda.synchronize()
    ref = R.colsum(x, c, alpha=0.75)
    _assert_within(out[:c], ref, _colsum_tol(x, c, 0.75, rows), f'colsum rows={rows} C={c}')
    assert torch.isnan(out[c]).item()
    base = torch.randn(c, generator=gen)
    acc = base.cuda()
    ops.colsum(xd, c, acc, alpha=0.75, accumulate=True)
    torch.cuda.synchronize()
    _assert_within(acc, ref + base.double(), _colsum_tol(x, c, 0.75, rows, base), f'colsum accumulate rows={rows} C={c}')


@pytest.mark.parametrize('row_perm', [2, 16])
def test_colsum_row_perm(row_perm):
    """row_perm: column j = k Cc + i of the [rows, C] input lands at out[i row_perm + k] (Cc = C / row_perm), as the
    generator's linear bias gradient reads its [16 positions x C] activation: here C = 16 x 8 = 128, 1000 rows, fp32 and bf16."""
    ops = _ops()
    gen = torch.Generator().manual_seed(row_perm)
    c = 128
    for dtype in (torch.float32, torch.bfloat16):
        x = (torch.randn(1000, c, generator=gen) + 0.5).to(dtype)
        out = torch.full((c,), NAN, device='cuda')
        ops.colsum(x.cuda(), c, out, alpha=2.0, row_perm=row_perm)
        torch.cuda.synchronize()
        tol = _colsum_tol(x, c, 2.0, 1000)
        tol = tol.view(row_perm, c // row_perm).t().reshape(-1)
        _assert_within(out, R.colsum(x, c, alpha=2.0, row_perm=row_perm), tol, f'row_perm {row_perm} {dtype}')
