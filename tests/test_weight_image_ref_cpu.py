"""weight_image_ref checked against itself, against torch's own tensor ops and against the library's host-side element
counts (no GPU): the references the GPU tests trust must agree with what the header documents."""
import ctypes

import numpy as np
import pytest
import torch

import weight_image_ref as R
from mcgen_amd import _lib
from test_wgrad_reduce_gpu import CASES as REDUCE_CASES, IDS as REDUCE_IDS

RAGGED = [(3, 1, 1), (16, 3, 3), (24, 8, 3), (130, 33, 3), (24, 40, 1), (16, 72, 3), (5, 130, 1)]


def _w(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('cout, cin, ks', RAGGED)
def test_unpack_inverts_image(cout, cin, ks, transpose):
    w = _w(cout, cin, ks, ks)
    img = R.image(w, ks, transpose=transpose)
    rows, kdim = (cin, cout) if transpose else (cout, cin)
    assert img.shape == (R.chunks(kdim), ks * ks, R.round_up(rows, 16), 32)
    assert np.array_equal(R.unpack(img, cout, cin, ks, transpose), w.numpy())
    assert np.count_nonzero(img) == w.numel()              # everything else is padding, and zero


@pytest.mark.parametrize('cout, cin, ks', RAGGED)
def test_transposed_image_is_the_forward_image_of_the_flipped_transposed_weight(cout, cin, ks):
    w = _w(cout, cin, ks, ks)
    assert np.array_equal(R.image(w, ks, transpose=True), R.image(w.transpose(0, 1).flip(2, 3), ks))


@pytest.mark.parametrize('row_perm', [2, 16])
def test_row_perm_reads_the_documented_master_row(row_perm):
    cout, cin = 32, 5
    w = _w(cout, cin, 3, 3)
    cc = cout // row_perm
    # image row co = k * Cc + i is master row i * row_perm + k: the [Cc, row_perm] view of the rows, transposed
    perm = w.view(cc, row_perm, cin, 3, 3).transpose(0, 1).reshape(cout, cin, 3, 3)
    assert np.array_equal(R.image(w, 3, row_perm=row_perm), R.image(perm, 3))
    assert np.array_equal(R.image(w, 3, row_perm=row_perm, transpose=True), R.image(perm, 3, transpose=True))


@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('kh, kw, kh0, kw0', [(2, 3, 0, 0), (1, 2, 1, 0), (1, 1, 1, 1)])
def test_embedded_window_is_the_zero_padded_weight(kh, kw, kh0, kw0, transpose):
    w = _w(24, 33, kh, kw)
    full = torch.zeros(24, 33, 3, 3, dtype=torch.float64)
    full[:, :, kh0:kh0 + kh, kw0:kw0 + kw] = w
    assert np.array_equal(R.image(w, 3, kh0=kh0, kw0=kw0, transpose=transpose), R.image(full, 3, transpose=transpose))


@pytest.mark.parametrize('transpose', [False, True])
@pytest.mark.parametrize('rows_img, k_img', [(40, None), (None, 16), (None, 64), (48, 64)])
def test_extent_padding_is_the_zero_padded_weight(rows_img, k_img, transpose):
    cout, cin = 12, 10
    w = _w(cout, cin, 3, 3)
    src_rows, src_k = (cin, cout) if transpose else (cout, cin)
    rows, kdim = rows_img or src_rows, k_img or src_k
    padded = torch.zeros((kdim, rows, 3, 3) if transpose else (rows, kdim, 3, 3), dtype=torch.float64)
    padded[:cout, :cin] = w
    assert np.array_equal(R.image(w, 3, rows_img=rows_img, k_img=k_img, transpose=transpose), R.image(padded, 3, transpose=transpose))


@pytest.mark.parametrize('transpose', [False, True])
def test_scales_index_the_source_channels(transpose):
    w, rs, cs = _w(24, 33, 3, 3), _w(24, seed=1), _w(33, seed=2)
    scaled = w * 0.5 * rs.view(-1, 1, 1, 1) * cs.view(1, -1, 1, 1)
    got = R.image(w, 3, scale=0.5, row_scale=rs, col_scale=cs, transpose=transpose)
    assert np.allclose(got, R.image(scaled, 3, transpose=transpose), rtol=1e-15, atol=0)


def test_kmap_and_rmap_gather_columns_and_rows():
    cout, cin = 24, 40
    w = _w(cout, cin, 3, 3)
    kmap = torch.tensor([5, 0, 39, 40, 7, -1, 12, 40] + [3] * 8, dtype=torch.int16)      # (entries past kcount are not read)
    rmap = torch.randperm(cout, generator=torch.Generator().manual_seed(3)).to(torch.int16)
    got = R.image(w, 3, kmap=kmap, kcount=8, rmap=rmap)
    cols = torch.zeros(cout, 8, 3, 3, dtype=torch.float64)
    for k, c in enumerate(kmap[:8].tolist()):
        if 0 <= c < cin:
            cols[:, k] = w[:, c]
    assert np.array_equal(got, R.image(cols[rmap.long()], 3))


@pytest.mark.parametrize('cout, cin, ks', RAGGED)
def test_image_k_layout(cout, cin, ks):
    w = _w(cout, cin, ks, ks)
    img = R.image_k(w, ks, 0.5)
    assert img.shape == (ks * ks, R.round_up(cin, 8) + 1, R.round_up(cout, 16))
    assert np.array_equal(img[:, :cin, :cout], 0.5 * w.reshape(cout, cin, ks * ks).permute(2, 1, 0).numpy())
    assert np.count_nonzero(img) == w.numel() and not img[:, -1].any()


@pytest.mark.parametrize('cout, cin, ks', RAGGED + [(528, 128, 1)])
def test_element_counts_agree_with_the_library(cout, cin, ks):
    lib = _lib.load()
    w = torch.zeros(cout, cin, ks, ks)
    for t in (False, True):
        assert R.image(w, ks, transpose=t).size == lib.mcgen_weight_image_elems(cout, cin, ks, int(t))
    assert R.image_k(w, ks).size == lib.mcgen_weight_image_k_elems(cout, cin, ks)
    assert R.image(w, ks, rows_img=cout + 20, k_img=cin + 30).size == lib.mcgen_weight_image_elems(cout + 20, cin + 30, ks, 0)


@pytest.mark.parametrize('case', REDUCE_CASES, ids=REDUCE_IDS)
def test_slab_element_counts_agree_with_the_library(case):
    lib = _lib.load()
    shape = R.slab_layout(case['Cout_w'], case['Cin'], case['cin_slab'], case['ksize'], case['tapcols'], case['Cout'])[0]
    p = _lib.Wgrad()
    p.seg.C, p.seg.ksize, p.Cout, p.Cout_w = case['cin_slab'] or case['Cin'], case['ksize'], case['Cout'], case['Cout_w']
    want = lib.mcgen_wgrad_c8_slab_elems(ctypes.byref(p)) if case['tapcols'] else lib.mcgen_wgrad_slab_elems(ctypes.byref(p))
    assert int(np.prod(shape)) == want


@pytest.mark.parametrize('case', REDUCE_CASES, ids=REDUCE_IDS)
def test_reduce_returns_a_gradient_split_into_random_parts(case):
    """Every addressing mode: a known [Cout][Cin][k * k] gradient, scattered into slabs whose sum it is (NaN in every
    dead entry), comes back -- permuted, scaled, windowed and accumulated as documented."""
    rng = np.random.default_rng(11)
    cout, cin, ks, cout_w, splits = case['Cout'], case['Cin'], case['ksize'], case['Cout_w'], case['splits']
    ntap = ks * ks
    layout = R.slab_layout(cout_w, cin, case['cin_slab'], ks, case['tapcols'], cout)
    known = rng.standard_normal((cout, cin, ntap))
    parts = rng.standard_normal((splits, cout, cin, ntap))
    parts[-1] = known - parts[:-1].sum(0)
    slabs = np.stack([R.scatter(p, layout, fill=np.nan) for p in parts])
    bias_known = rng.standard_normal(cout)
    bparts = rng.standard_normal((splits * 4, cout_w))
    bparts[-1, :cout] = bias_known - bparts[:-1, :cout].sum(0)
    bparts[:, cout:] = np.nan
    rs = rng.uniform(0.5, 2.0, cout) if case['row_scale'] else None
    tap0, nout = case['win'] if case['win'] and case['win'][1] else (0, ntap)
    prev = rng.standard_normal((cout, cin, nout)) if case['accumulate'] else None
    out = R.reduce(slabs, cout, cin, ks, cout_w, cin_slab=case['cin_slab'], tapcols=case['tapcols'], alpha=0.75, row_scale=rs,
                   row_perm=case['row_perm'], accumulate=prev, tap0=case['win'][0] if case['win'] else 0,
                   ntap_out=case['win'][1] if case['win'] else 0, bias_slabs=bparts)
    # slab row co lands in master row (co % Cc) * row_perm + co // Cc, scaled by that MASTER row's row_scale
    rows = np.arange(cout)
    if case['row_perm'] > 1:
        cc = cout // case['row_perm']
        rows = (rows % cc) * case['row_perm'] + rows // cc
    want = np.zeros((cout, cin, nout))
    want[rows] = known[:, :, tap0:tap0 + nout]
    want_bias = np.zeros(cout)
    want_bias[rows] = bias_known
    f = 0.75 * (rs if rs is not None else np.ones(cout))
    want, want_bias = want * f[:, None, None], want_bias * f
    if prev is not None:
        want = want + prev
    assert out['grad'].shape == (cout, cin, nout)
    assert np.allclose(out['grad'], want, rtol=0, atol=1e-11 * splits)
    assert np.allclose(out['bias'], want_bias, rtol=0, atol=1e-11 * splits)
    assert np.isfinite(out['sum_abs']).all() and (out['sum_abs'] * np.abs(f)[:, None, None] + 1e-9 >= np.abs(want - (prev if prev is not None else 0))).all()
