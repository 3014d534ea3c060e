"""Float64 CPU restatements of the weight-image builders (csrc/small_ops.hip: mcgen_prep_weight, _rows, _ex, _batch, _k)
and of the split-K slab reduce (csrc/wgrad.hip: mcgen_wgrad_reduce).  Everything is stated from the layouts that
include/mcgen_hip.h documents, as whole-array index arithmetic: an image is a gather from the zero-padded master weight
through three index vectors (rows, K columns, taps), a slab is a scatter of the master-layout gradient through the map
slab_layout returns.  test_weight_image_ref_cpu.py checks these functions against each other and against the library's
host-side element counts; test_weight_image_gpu.py and test_wgrad_reduce_gpu.py check the kernels against them.

Scalars are taken at face value: pass the fp32 value a kernel received (f32(1.7)), and wscale / sigma as the float64
quotient of the two fp32 values."""
import numpy as np
import torch

CK = 32          # MCGEN_CK: K columns per chunk of an image or a slab


def f32(x: float) -> float:
    """The fp32 value a kernel receives for the Python float x."""
    return float(np.float32(x))


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def chunks(k: int) -> int:
    """Chunks of 32 K columns that hold k columns: k rounded up to 8, then to 32."""
    return round_up(round_up(k, 8), CK) // CK


def _np64(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().to(torch.float64).numpy()
    return np.asarray(t, dtype=np.float64)


def _ints(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.int64)


def master_row(co, Cout: int, row_perm: int):
    """Master row of image / slab row co: (co % Cc) * row_perm + co // Cc with Cc = Cout // row_perm."""
    if row_perm <= 1:
        return co
    cc = Cout // row_perm
    return (co % cc) * row_perm + co // cc


def image(w, ksize=None, *, transpose=False, row_perm=1, scale=1.0, rows_img=None, k_img=None, kh0=0, kw0=0,
          row_scale=None, col_scale=None, kmap=None, kcount=0, rmap=None):
    """Chunked weight image [chunk][tap][rows_w][32] (float64) of the master weight w [Cout, Cin(, KH, KW)].

    The source taps sit at (kh0, kw0) of a ksize x ksize filter (zero elsewhere) and are multiplied by
    scale * row_scale[co] * col_scale[ci], co / ci being SOURCE indices in both orientations.  Forward: rows = Cout,
    K = Cin.  transpose: rows = Cin, K = Cout, tap (kh, kw) taken from (ksize-1-kh, ksize-1-kw).  Image output channel co
    reads master row master_row(rmap[co] if rmap else co).  kmap: K column k < kcount is source channel kmap[k]; an entry
    outside [0, Cin) is a zero column.  rows_img / k_img set the image's extents (zero outside the source)."""
    w = _np64(w)
    if w.ndim == 2:
        w = w[:, :, None, None]
    Cout, Cin, KH, KW = w.shape
    ks = KH if ksize is None else ksize
    assert kh0 >= 0 and kw0 >= 0 and kh0 + KH <= ks and kw0 + KW <= ks
    src = w * float(scale)
    if row_scale is not None:
        src = src * _np64(row_scale).reshape(Cout, 1, 1, 1)
    if col_scale is not None:
        src = src * _np64(col_scale).reshape(1, Cin, 1, 1)
    # the ksize x ksize filter, one extra all-zero output row / input channel / tap at index -1 for dead positions
    full = np.zeros((Cout + 1, Cin + 1, ks * ks + 1))
    emb = np.zeros((Cout, Cin, ks, ks))
    emb[:, :, kh0:kh0 + KH, kw0:kw0 + KW] = src
    full[:Cout, :Cin, :ks * ks] = emb.reshape(Cout, Cin, ks * ks)

    co_n = Cout                                            # output channels / input channels the image can address
    ci_n = kcount if kmap is not None else Cin
    rows = (ci_n if transpose else co_n) if rows_img is None else rows_img
    kdim = (co_n if transpose else ci_n) if k_img is None else k_img
    rows_w, nq = round_up(rows, 16), chunks(kdim)

    def co_index(n_img, width):                            # image output channel -> master row, -1 dead
        i = np.arange(width)
        live = (i < n_img) & (i < Cout)
        j = np.where(live, i, 0)
        if rmap is not None:
            j = _ints(rmap)[:Cout][np.minimum(j, Cout - 1)]
        j = master_row(j, Cout, row_perm)
        return np.where(live, j, -1)

    def ci_index(n_img, width):                            # image input channel -> source channel, -1 dead
        i = np.arange(width)
        live = (i < n_img) & (i < ci_n)
        j = np.where(live, i, 0)
        if kmap is not None:
            j = _ints(kmap)[np.minimum(j, ci_n - 1)]
            live = live & (j >= 0) & (j < Cin)
        return np.where(live, j, -1)

    taps = np.arange(ks * ks)
    if transpose:
        assert kmap is None and rmap is None
        taps = (ks - 1 - taps // ks) * ks + (ks - 1 - taps % ks)
        r_idx, k_idx = ci_index(rows, rows_w), co_index(kdim, nq * CK)
        g = full[k_idx][:, r_idx][:, :, taps]              # [K, rows, tap]
        g = g.transpose(1, 0, 2)
    else:
        r_idx, k_idx = co_index(rows, rows_w), ci_index(kdim, nq * CK)
        g = full[r_idx][:, k_idx][:, :, taps]              # [rows, K, tap]
    return np.ascontiguousarray(g.reshape(rows_w, nq, CK, ks * ks).transpose(1, 3, 0, 2))


def image_k(w, ksize=None, scale=1.0):
    """K-major image [tap][round_up(Cin, 8) + 1][round_up(Cout, 16)] (float64): element (tap, ci, co) = w[co, ci, tap] * scale,
    zero padding, and a trailing all-zero K row."""
    w = _np64(w)
    if w.ndim == 2:
        w = w[:, :, None, None]
    Cout, Cin, KH, KW = w.shape
    assert KH == KW and (ksize is None or ksize == KH)
    out = np.zeros((KH * KW, round_up(Cin, 8) + 1, round_up(Cout, 16)))
    out[:, :Cin, :Cout] = (w * float(scale)).reshape(Cout, Cin, KH * KW).transpose(2, 1, 0)
    return out


def unpack(img, Cout: int, Cin: int, ksize: int, transpose=False):
    """The master weight [Cout, Cin, k, k] read back out of a plain forward or transposed chunked image."""
    img = _np64(img)
    rows, kdim = (Cin, Cout) if transpose else (Cout, Cin)
    img = img.reshape(chunks(kdim), ksize * ksize, round_up(rows, 16), CK)
    co, ci, kh, kw = np.meshgrid(np.arange(Cout), np.arange(Cin), np.arange(ksize), np.arange(ksize), indexing='ij')
    if transpose:
        return img[co // CK, (ksize - 1 - kh) * ksize + (ksize - 1 - kw), ci, co % CK]
    return img[ci // CK, kh * ksize + kw, co, ci % CK]


def slab_layout(Cout_w: int, Cin: int, cin_slab: int, ksize: int, tapcols: int, Cout=None):
    """One split's slab of a weight-gradient launch: (shape, co, ci, tap), the three maps being int arrays of that shape
    that name the gradient element a slab entry holds, or -1 where the entry is dead (a padding row >= Cout, a column
    >= Cin, the padding of cin_slab, a compact column whose tap >= k * k).

    Plain slabs are [chunks(cin_slab or Cin)][k * k][Cout_w][32] with column = ci % 32 of chunk ci // 32.  tapcols
    (the image layer's compact slabs) are [ceil(k * k * 8 / 32)][Cout_w][32] with column tap * 8 + ci."""
    Cout = Cout_w if Cout is None else Cout
    ntap = ksize * ksize
    if tapcols:
        assert Cin <= 8 and cin_slab in (0, 8)
        nq = (ntap * 8 + CK - 1) // CK
        q, co, cl = np.meshgrid(np.arange(nq), np.arange(Cout_w), np.arange(CK), indexing='ij')
        col = q * CK + cl
        tap, ci = col // 8, col % 8
    else:
        cs = cin_slab if cin_slab > 0 else Cin
        assert cs >= Cin
        q, tap, co, cl = np.meshgrid(np.arange(chunks(cs)), np.arange(ntap), np.arange(Cout_w), np.arange(CK), indexing='ij')
        ci = q * CK + cl
    live = (co < Cout) & (ci < Cin) & (tap < ntap)
    return co.shape, np.where(live, co, -1), np.where(live, ci, -1), np.where(live, tap, -1)


def scatter(master, layout, fill=0.0):
    """A slab (float64, layout's shape) that holds the plain [Cout][Cin][k * k] gradient `master` (slab row co = gradient
    row co: no row_perm), `fill` in every dead entry."""
    shape, co, ci, tap = layout
    master = _np64(master)
    live = co >= 0
    out = np.full(shape, float(fill))
    out[live] = master.reshape(master.shape[0], master.shape[1], -1)[co[live], ci[live], tap[live]]
    return out


def reduce(slabs, Cout: int, Cin: int, ksize: int, Cout_w: int, *, cin_slab=0, tapcols=0, alpha=1.0, row_scale=None,
           row_perm=1, accumulate=None, tap0=0, ntap_out=0, bias_slabs=None, bias_accumulate=None):
    """mcgen_wgrad_reduce in float64.  slabs: [splits, *slab shape]; accumulate: the previous gradient or None.

    -> dict: grad [Cout][Cin][ntap_out or k * k] = (previous +) alpha * row_scale[row] * sum over splits, slab row co stored
    at master_row(co) (row_scale indexes the master row), taps tap0 .. tap0 + ntap_out - 1 only when ntap_out > 0;
    sum_abs, the same sum over |slab| without alpha, row_scale or the previous value; bias / bias_sum_abs [Cout] from
    bias_slabs [splits * 4][Cout_w] in the same way (None without bias_slabs)."""
    slabs = _np64(slabs)
    shape, co, ci, tap = slab_layout(Cout_w, Cin, cin_slab, ksize, tapcols, Cout)
    assert slabs.shape[1:] == shape, (slabs.shape, shape)
    ntap = ksize * ksize
    nout = ntap_out if ntap_out > 0 else ntap
    t0 = tap0 if ntap_out > 0 else 0
    assert 0 <= t0 and t0 + nout <= ntap
    take = (co >= 0) & (tap >= t0) & (tap < t0 + nout)
    rs = np.ones(Cout) if row_scale is None else _np64(row_scale).reshape(Cout)
    com = master_row(co[take], Cout, row_perm)
    total = np.where(take, slabs, 0.0).sum(0)              # (dead entries may hold NaN: they take no part)
    total_abs = np.where(take, np.abs(slabs), 0.0).sum(0)
    grad = np.zeros((Cout, Cin, nout))
    sum_abs = np.zeros((Cout, Cin, nout))
    grad[com, ci[take], tap[take] - t0] = float(alpha) * rs[com] * total[take]
    sum_abs[com, ci[take], tap[take] - t0] = total_abs[take]
    if accumulate is not None:
        grad = grad + _np64(accumulate).reshape(grad.shape)
    out = {'grad': grad, 'sum_abs': sum_abs, 'bias': None, 'bias_sum_abs': None}
    if bias_slabs is not None:
        b = _np64(bias_slabs)
        assert b.shape == (slabs.shape[0] * 4, Cout_w)
        rows = master_row(np.arange(Cout), Cout, row_perm)
        bias, babs = np.zeros(Cout), np.zeros(Cout)
        bias[rows] = float(alpha) * rs[rows] * b[:, :Cout].sum(0)
        babs[rows] = np.abs(b[:, :Cout]).sum(0)
        if bias_accumulate is not None:
            bias = bias + _np64(bias_accumulate).reshape(Cout)
        out['bias'], out['bias_sum_abs'] = bias, babs
    return out
