"""Tensor-level wrappers over the C ABI (include/mcgen_hip.h).

Activations are torch tensors of shape [N, H, W, Cp] (channels last, Cp a
multiple of 8), dtype float32 or bfloat16, on a ROCm device.  All launches go
to torch's current stream, so they compose with torch.cuda.graphs and streams.
Nothing here has a CPU path: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C
import os as _os
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check
from ._tuning import flag as _flag

Tensor = torch.Tensor


def _dt(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return _lib.F32
    if dtype == torch.bfloat16:
        return _lib.BF16
    raise _lib.McgenError(f'unsupported compute dtype {dtype}')


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.McgenError('mcgen_amd has no CPU path: tensor is not on a ROCm device')
    if not t.is_contiguous():
        raise _lib.McgenError('mcgen_amd kernels need contiguous tensors')
    return t.data_ptr()


def _f32(t: Optional[Tensor]) -> Optional[int]:
    if t is not None and t.dtype != torch.float32:
        raise _lib.McgenError(f'expected float32, got {t.dtype}')
    return _p(t)


# ---- per-launch profiling (bench.py roofline): HIP events on the launch stream -------------------------
_PROF = None
_PROF_SHAPES = _flag('MCGEN_PROF_SHAPES', '') != ''      # per-shape kernel names in the profile (tools/shape_table.py)
TILE_LOG = None        # tests set this to a list: every conv_fused launch appends the (BM, BN) tile the policy picked
FORM_LOG = None        # tests set this to a list: every conv_fused launch appends its weight layout (0 dense, 1 mc, 2 gk)
KERNEL_LOG = None      # tests set this to a list: every conv_fused launch appends mcgen_conv_form (0 tiled, 1 skinny, 2 whole images per workgroup, 3 resident-tile 1x1, 4 image convolution, 5 image head)


def _timed(name_fn, flops: float, launch, nbytes_fn=None, extra_fn=None):
    """Run `launch()`; when profiling is on, bracket it with events on the current stream.  `nbytes_fn()` = the
    launch's ALGORITHMIC HBM bytes (operands read once + results written once); `extra_fn()` = bytes the implementation
    moves on top of that (the split-K slabs of a weight-gradient launch), reported apart."""
    if _PROF is None:
        return launch()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    r = launch()
    e.record()
    _PROF.append((name_fn(), flops, s, e, float(nbytes_fn()) if nbytes_fn is not None else 0.0,
                  float(extra_fn()) if extra_fn is not None else 0.0))
    return r


HBM_PEAK_BYTES_PER_S = 8.0e12      # MI355X_MICROARCH.md: HBM3E spec peak


def _nbytes(*ts) -> int:
    return sum(t.numel() * t.element_size() for t in ts if t is not None)


def profile_step(fn, peak_tflops: float, iters: int = 5):
    """Run `fn` once untimed, then `iters` times with every conv / wgrad / slab-reduce launch bracketed by HIP events on
    the launch stream; returns the `roofline` object for the kernel instantiation with the largest total time:
    algorithmic FLOPs of its launches / sum of their measured durations, averaged over all `iters` passes, with the
    per-pass fractions' min / median beside it (`fn(i)` is called with the pass index if it takes an argument)."""
    global _PROF
    import inspect
    takes_i = len(inspect.signature(fn).parameters) >= 1
    call = (lambda i: fn(i)) if takes_i else (lambda i: fn())
    call(-1)
    torch.cuda.synchronize()
    recs = []
    for i in range(max(1, iters)):
        _PROF = []
        try:
            call(i)
            torch.cuda.synchronize()
            recs.append(_PROF)
        finally:
            _PROF = None
    # An event pair with nothing between its records already reads ~4.8 us on this stack (the second event's own
    # completion); measured live and taken off every bracket, otherwise short launches look 10-15 % slower than rocprofv3's
    # kernel durations (checked: 55.2 -> 50.4 us against 48.2 us for the 128x128 tile, 163.3 -> 158.5 against 159.3).
    pairs = []
    for _ in range(64):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); e.record(); pairs.append((s, e))
    torch.cuda.synchronize()
    over_ms = sorted(s.elapsed_time(e) for s, e in pairs)[len(pairs) // 2]

    def aggregate(rec):
        agg = {}
        for name, flops, s, e, nbytes, extra in rec:
            a = agg.setdefault(name, [0, 0.0, 0.0, 0.0, 0.0, 0.0])
            raw = s.elapsed_time(e)
            a[0] += 1; a[1] += max(raw - over_ms, 0.1 * raw) * 1e-3; a[2] += flops; a[3] += raw * 1e-3; a[4] += nbytes; a[5] += extra
        return agg
    per_pass = [aggregate(r) for r in recs]
    agg = {}
    for pa in per_pass:
        for k, v in pa.items():
            a = agg.setdefault(k, [0, 0.0, 0.0, 0.0, 0.0, 0.0])
            for j in range(6):
                a[j] += v[j]
    if not agg:
        return None
    np_ = len(per_pass)
    top = max(agg, key=lambda k: agg[k][1])
    cnt, secs, flops, raw_secs, nbytes, extra = agg[top]
    ach = flops / secs / 1e12
    # which roof bounds the kernel: its algorithmic intensity against the machine balance (MFMA peak / HBM peak)
    intensity = flops / nbytes if nbytes > 0 else float('inf')
    balance = peak_tflops * 1e12 / HBM_PEAK_BYTES_PER_S
    hbm = intensity < balance
    # the same figure per pass: how reproducible one eager iteration's reading is
    fr = sorted(((pa[top][4] / pa[top][1] / HBM_PEAK_BYTES_PER_S) if hbm else (pa[top][2] / pa[top][1] / 1e12 / peak_tflops))
                for pa in per_pass if top in pa and pa[top][1] > 0)
    out = {'bound': 'hbm' if hbm else 'mfma', 'kernel': top, 'achieved': ach, 'peak': peak_tflops,
           'unit': 'TFLOP/s', 'frac': ach / peak_tflops, 'traffic': None, 'launches_per_step': cnt / np_,
           'passes': np_, 'frac_min': fr[0], 'frac_median': fr[len(fr) // 2], 'frac_max': fr[-1],
           'avg_launch_us': secs / cnt * 1e6, 'avg_launch_us_uncorrected': raw_secs / cnt * 1e6,
           'event_pair_overhead_us': over_ms * 1e3, 'flops_per_launch': flops / cnt,
           'algorithmic_bytes_per_launch': nbytes / cnt, 'split_k_bytes_per_launch': extra / cnt,
           'intensity_flop_per_byte': intensity, 'machine_balance_flop_per_byte': balance,
           'by_kernel': {k: {'launches': v[0] / np_, 'total_ms': v[1] * 1e3 / np_, 'tflops': v[2] / v[1] / 1e12,
                             'gbytes_per_s': v[4] / v[1] / 1e9, **({'split_k_gbytes_per_s': v[5] / v[1] / 1e9} if v[5] else {})}
                         for k, v in sorted(agg.items(), key=lambda kv: -kv[1][1])}}
    if hbm:                                        # an HBM-bound dominant kernel is priced in bytes
        out.update(achieved=nbytes / secs / 1e9, peak=HBM_PEAK_BYTES_PER_S / 1e9, unit='GB/s',
                   frac=nbytes / secs / HBM_PEAK_BYTES_PER_S)
    return out


def pad8(c: int) -> int:
    return (c + 7) // 8 * 8


def pad16(c: int) -> int:
    return (c + 15) // 16 * 16


@dataclass
class Seg:
    """One K-segment of a fused convolution (mcgen_seg_t)."""
    x: Tensor                       # [N, H>>ups, W>>ups, C]
    ksize: int = 3
    scale: Optional[Tensor] = None  # BN affine
    shift: Optional[Tensor] = None
    code: Optional[Tensor] = None   # [N, C] MC code
    ups: bool = False
    relu: bool = False
    group_n: int = 0                # > 0: scale / shift are [N // group_n, C], one BatchNorm batch per group_n images
    cmap: Optional[Tensor] = None   # int16 [N, cmap_stride(C)] compaction map of `code` (mc_cmap): mode-compacted K loop
    cw: int = 0                     # kmajor=2: channels of the segment's WEIGHTS when x holds compacted channels (else 0)

    def fill(self, s: _lib.Seg):
        s.x = _p(self.x)
        s.scale, s.shift, s.code = _f32(self.scale), _f32(self.shift), _f32(self.code)
        s.C = self.x.shape[-1]
        s.ups, s.relu, s.ksize = int(self.ups), int(self.relu), self.ksize
        s.group_n = int(self.group_n)
        s.cmap, s.cmap_stride, s.Cw = None, 0, int(self.cw)
        if self.cmap is not None:
            cm = self.cw or s.C                                 # the map is over the weights' (true) channels
            if self.cmap.dtype != torch.int16 or tuple(self.cmap.shape) != (self.x.shape[0], cmap_stride(cm)):
                raise _lib.McgenError(f'cmap must be int16 {(self.x.shape[0], cmap_stride(cm))}, got {self.cmap.dtype} {tuple(self.cmap.shape)}')
            s.cmap, s.cmap_stride = _p(self.cmap), self.cmap.shape[1]
        if self.group_n and self.scale is not None:
            g = self.x.shape[0] // self.group_n
            if self.x.shape[0] % self.group_n or tuple(self.scale.shape) != (g, s.C) or tuple(self.shift.shape) != (g, s.C):
                raise _lib.McgenError(f'grouped BatchNorm affine must be {(g, s.C)}, got {tuple(self.scale.shape)}')
        if self.code is not None and tuple(self.code.shape) != (self.x.shape[0], self.x.shape[-1]):
            raise _lib.McgenError(f'code shape {tuple(self.code.shape)} does not match x {tuple(self.x.shape)}')


# --------------------------------------------------------------------------- #
def to_nhwc(x: Tensor, dtype: torch.dtype, cp: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """NCHW fp32 -> NHWC `dtype`, channels zero-padded to a multiple of 8 (`out`: a contiguous [N, H, W, cp] buffer to fill)."""
    n, c, h, w = x.shape
    cp = cp or pad8(c)
    y = out if out is not None else torch.empty((n, h, w, cp), dtype=dtype, device=x.device)
    if tuple(y.shape) != (n, h, w, cp) or y.dtype != dtype or not y.is_contiguous():
        raise _lib.McgenError(f'to_nhwc: out must be a contiguous {(n, h, w, cp)} {dtype} tensor')
    check(_lib.load().mcgen_nchw_to_nhwc(_f32(x.contiguous()), _p(y), _dt(dtype), n, c, h, w, cp, _stream()), 'nchw_to_nhwc')
    return y


def to_nchw(x: Tensor, c: int) -> Tensor:
    n, h, w, cp = x.shape
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    check(_lib.load().mcgen_nhwc_to_nchw(_p(x), _f32(y), _dt(x.dtype), n, c, h, w, cp, _stream()), 'nhwc_to_nchw')
    return y


def pool2_sum(x: Tensor) -> Tensor:
    """2x2 sums of an NHWC tensor (adjoint of the nearest x2 upsample)."""
    n, h, w, c = x.shape
    y = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
    check(_lib.load().mcgen_pool2_sum(_p(x), _p(y), _dt(x.dtype), n, h // 2, w // 2, c, _stream()), 'pool2_sum')
    return y


def mc_code(indicator: Tensor, codebook: Tensor, cp: Optional[int] = None) -> Tensor:
    """code = indicator @ codebook  (modules.py:73), zero-padded to `cp` columns."""
    n, m = indicator.shape
    c = codebook.shape[1]
    code = torch.empty((n, c), dtype=torch.float32, device=indicator.device)
    check(_lib.load().mcgen_mc_code(_f32(indicator.contiguous()), _f32(codebook.contiguous()), _f32(code), n, m, c, _stream()), 'mc_code')
    if cp is not None and cp != c:
        code = torch.nn.functional.pad(code, (0, cp - c))
    return code


def mc_apply(x: Tensor, code: Tensor, channels_last: bool = True) -> Tensor:
    """x * code; x is [N, ..., C] (channels_last) or [N, C, ...] (the reference's layout)."""
    n = x.shape[0]
    c = x.shape[-1] if channels_last else x.shape[1]
    hw = x.numel() // (n * c)
    y = torch.empty_like(x)
    check(_lib.load().mcgen_mc_apply(_p(x), _f32(code), _p(y), _dt(x.dtype), n, hw, c, int(channels_last), _stream()), 'mc_apply')
    return y


def _conv_plan(p: '_lib.Conv', dtype: torch.dtype) -> '_lib.ConvPlan':
    """What mcgen_conv_fused will do with `p` (mcgen_conv_plan: the launch makes this same plan): the launcher, its tile, the
    rows of `stats`.  Raises where the launch would refuse `p`; asked before `stats` exists."""
    plan = _lib.ConvPlan()
    check(_lib.load().mcgen_conv_plan(C.byref(p), _dt(dtype), C.byref(plan)), 'conv_fused')
    return plan


def tile_images(n: int, h: int, w: int, cout: int, dtype: torch.dtype) -> int:
    """Images per output tile of a fused convolution over an [n, h, w] map with `cout` output channels, as the
    launcher's tile policy picks it (1 when a tile lies inside one image)."""
    p = _lib.Conv()
    p.nseg, p.N, p.H, p.W, p.Cout, p.Cout_w, p.Cy = 1, n, h, w, cout, pad16(cout), pad8(cout)
    # a plain 8-channel 1x1 segment: no kernel outside the tile table takes it, so the plan names the policy's tile
    # (the buffers are placeholders that nothing dereferences: the plan only asks whether they are set)
    p.seg[0].C, p.seg[0].ksize = 8, 1
    p.seg[0].x = p.w = p.y = 1
    return max(1, _conv_plan(p, dtype).bm // (h * w))


def cmap_stride(c: int) -> int:
    return int(_lib.load().mcgen_cmap_stride(c))


def onehot_rep(label: Tensor, classes: int, reps: int, out: Optional[Tensor] = None, lab32: Optional[Tensor] = None) -> Tensor:
    """[reps * N, classes] fp32: F.one_hot(label, classes).float() (mcgan.py:196,201) `reps` times back to back, one launch.
    `lab32` (optional, int32 [reps * N]) receives the labels themselves, repeated (the per-image weight-set index of conv_fused)."""
    n = label.shape[0]
    if label.dtype != torch.int64 or not label.is_cuda:
        raise _lib.McgenError('onehot_rep: int64 labels on the GPU')
    if out is None:
        out = torch.empty((reps * n, classes), dtype=torch.float32, device=label.device)
    assert tuple(out.shape) == (reps * n, classes) and out.dtype == torch.float32 and out.is_contiguous()
    if lab32 is not None:
        assert lab32.dtype == torch.int32 and lab32.numel() == reps * n and lab32.is_contiguous()
    check(_lib.load().mcgen_onehot_rep(_p(label.contiguous()), _f32(out), _p(lab32), n, classes, reps, _stream()), 'onehot_rep')
    return out


def onehot_hint(indicator: Tensor, label: Tensor, reps: int = 1, lab32: Optional[Tensor] = None) -> Tensor:
    """Marks `indicator` ([reps * N, modes]) as F.one_hot(label) repeated `reps` times: CodeBatch.run_any then gathers codebook
    rows by label instead of multiplying through every mode (the tensor is returned; the mark does not survive slicing)."""
    indicator._mcgen_onehot = (label, int(reps), lab32)
    return indicator


def mc_cmap(code: Tensor) -> Tensor:
    """Per-sample compaction map of a code tensor [N, C] (mcgen_mc_cmap): int16 [N, cmap_stride(C)]."""
    n, c = code.shape
    out = torch.empty((n, cmap_stride(c)), dtype=torch.int16, device=code.device)
    check(_lib.load().mcgen_mc_cmap(_f32(code), n, c, _p(out), _stream()), 'mc_cmap')
    return out


def mc_affine(code: Tensor, cmap: Tensor, ccap: int, scale: Optional[Tensor] = None, shift: Optional[Tensor] = None,
              group_n: int = 0):
    """Per-image prologue rows [N, ccap] of a launch that reads compacted activations (mcgen_mc_affine): the
    BatchNorm affine (scale / shift: [C] or [N // group_n, C]) gathered through the map and multiplied by the code."""
    n, c = code.shape
    out = torch.empty((2, n, ccap), dtype=torch.float32, device=code.device)
    check(_lib.load().mcgen_mc_affine(_f32(scale), _f32(shift), group_n, _f32(code), _p(cmap), n, c, ccap,
                                      out[0].data_ptr(), out[1].data_ptr(), _stream()), 'mc_affine')
    return out[0], out[1]


def weight_image_k_elems(cout: int, cin: int, ksize: int) -> int:
    return int(_lib.load().mcgen_weight_image_k_elems(cout, cin, ksize))


def prep_weight_k(w: Tensor, dtype: torch.dtype, sigma: Optional[Tensor] = None, wscale: float = 1.0,
                  out: Optional[Tensor] = None) -> Tensor:
    """Master weights [Cout, Cin, k, k] -> K-major image [tap][round_up(Cin, 8) + 1][pad16(Cout)] (last row zero)."""
    cout, cin = w.shape[0], w.shape[1]
    ks = w.shape[2] if w.dim() == 4 else 1
    n = weight_image_k_elems(cout, cin, ks)
    if out is None:
        out = torch.empty(n, dtype=dtype, device=w.device)
    assert out.numel() == n and out.dtype == dtype
    check(_lib.load().mcgen_prep_weight_k(_f32(w.contiguous()), _p(out), _dt(dtype), cout, cin, ks, _f32(sigma), float(wscale), _stream()),
          'prep_weight_k')
    return out


def weight_image_elems(cout: int, cin: int, ksize: int, transpose: bool = False) -> int:
    return int(_lib.load().mcgen_weight_image_elems(cout, cin, ksize, int(transpose)))


def prep_weight(w: Tensor, dtype: torch.dtype, transpose: bool = False, row_perm: int = 1,
                sigma: Optional[Tensor] = None, wscale: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    """Master weights [Cout, Cin, k, k] (or [Cout, Cin]) -> kernel weight image."""
    cout, cin = w.shape[0], w.shape[1]
    ks = w.shape[2] if w.dim() == 4 else 1
    n = weight_image_elems(cout, cin, ks, transpose)
    if out is None:
        out = torch.empty(n, dtype=dtype, device=w.device)
    assert out.numel() == n and out.dtype == dtype
    check(_lib.load().mcgen_prep_weight(_f32(w), _p(out), _dt(dtype), cout, cin, ks, int(transpose), row_perm,
                                        _f32(sigma), float(wscale), _stream()), 'prep_weight')
    return out


def conv_fused(segs: Sequence[Seg], wimg: Tensor, cout: int, *, bias: Optional[Tensor] = None, bias2: Optional[Tensor] = None,
               pool: bool = False, alpha: float = 1.0, res: Optional[Tensor] = None,
               ocode: Optional[Tensor] = None, gate_x: Optional[Tensor] = None,
               gscale: Optional[Tensor] = None, gshift: Optional[Tensor] = None,
               gmean: Optional[Tensor] = None, grstd: Optional[Tensor] = None,
               tanh: bool = False, stats_mode: int = 0, cy: Optional[int] = None,
               out: Optional[Tensor] = None, kmajor: int = 0, ycmap: Optional[Tensor] = None,
               y_group: int = 0, wsel: Optional[Tensor] = None, order: Optional[Tensor] = None,
               yperm: Optional[Tensor] = None, wlive: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """Launch mcgen_conv_fused; returns (y, per-tile stats partials or None).  `kmajor`: `wimg` is the K-major image
    (prep_weight_k, segments concatenated); 1: every segment carries a compaction map and is compacted while staged;
    2: segments hold ALREADY compacted channels (Seg.cw, cmap) or are dense.  `ycmap` (+ `cy` = compacted pitch): the
    output keeps, per image, only the channels of that map, compacted (forward-only passes).  `y_group` (image head only):
    `out` holds 2 N images and output image n lands in slot (n // y_group) * 2 * y_group + y_group + n % y_group -- the
    second halves of N / y_group paired [real (+) generated] batches (mcgen_conv_t.y_group).
    `wsel` (int32 [N]) + `order` (int32 [N], a permutation; optional): per-mode dense weight sets -- `wimg` holds S images of
    the segments' (compacted) shapes back to back, the image walked at position i is order[i] and multiplies weight set
    wsel[i] (mcgen_conv_t.wsel: bf16, software-pipelined form only).  `yperm` (int16 [S, stride], with wsel and `cy`): the sets'
    weight ROWS were permuted at prep time (PrepBatch rmap = yperm[s]): the output comes out compacted (pitch cy) without a
    gather pass; bias and statistics stay in true channel order (mcgen_conv_t.yperm).  `wlive` (int32 [S, len(segs)], with
    wsel): the live 32-channel chunks of every segment of every set -- a tile stops its K loops there (mcgen_conv_t.wlive)."""
    s0 = segs[0]
    n = s0.x.shape[0]
    h = s0.x.shape[1] * (2 if s0.ups else 1)
    w = s0.x.shape[2] * (2 if s0.ups else 1)
    dtype = s0.x.dtype
    cy = cy or pad8(cout)
    ho, wo = (h // 2, w // 2) if pool else (h, w)
    p = _lib.Conv()
    p.nseg = len(segs)
    for i, s in enumerate(segs):
        if s.x.dtype != dtype:
            raise _lib.McgenError('all segments must share the compute dtype')
        hs = s.x.shape[1] * (2 if s.ups else 1)
        if hs != h or s.x.shape[0] != n:
            raise _lib.McgenError('segments disagree on the convolution resolution')
        s.fill(p.seg[i])
    if wimg.dtype != dtype:
        raise _lib.McgenError(f'weight image dtype {wimg.dtype} != activation dtype {dtype}')
    if kmajor:
        need = sum(s.ksize * s.ksize * ((s.cw or s.x.shape[-1]) + 1) for s in segs) * pad16(cout)
    else:
        need = sum(((s.x.shape[-1] + 31) // 32) * s.ksize * s.ksize for s in segs) * pad16(cout) * 32
    if wsel is not None:
        if wsel.dtype != torch.int32 or wsel.numel() != n or (order is not None and (order.dtype != torch.int32 or order.numel() != n)):
            raise _lib.McgenError('wsel / order must be int32 [N]')
        if wimg.numel() % need:
            raise _lib.McgenError(f'weight sets: {wimg.numel()} elements are not a multiple of one image ({need})')
    elif order is not None:
        raise _lib.McgenError('order comes with wsel')
    elif wimg.numel() != need:
        raise _lib.McgenError(f'weight image has {wimg.numel()} elements, the segments need {need}')
    y = out if out is not None else torch.empty((n, ho, wo, cy), dtype=dtype, device=s0.x.device)
    if y_group:
        if out is None or tuple(y.shape) != (2 * n, ho, wo, cy) or y.dtype != dtype or not y.is_contiguous():
            raise _lib.McgenError(f'y_group: `out` must be a contiguous {(2 * n, ho, wo, cy)} {dtype} buffer')
    else:
        assert tuple(y.shape) == (n, ho, wo, cy) and y.dtype == dtype
    p.w, p.bias, p.y = _p(wimg), _f32(bias), _p(y)
    p.bias2 = _f32(bias2)
    p.N, p.H, p.W = n, h, w
    p.Cout, p.Cout_w, p.Cy = cout, pad16(cout), cy
    p.pool, p.alpha = int(pool), float(alpha)
    for name, t in (('res', res), ('gate_x', gate_x)):
        if t is not None and (tuple(t.shape) != (n, ho, wo, cy) or t.dtype != dtype):
            raise _lib.McgenError(f'{name} must be {(n, ho, wo, cy)} {dtype}, got {tuple(t.shape)} {t.dtype}')
    if ocode is not None and tuple(ocode.shape) != (n, cout):
        raise _lib.McgenError(f'ocode must be {(n, cout)}')
    p.res, p.ocode, p.gate_x = _p(res), _f32(ocode), _p(gate_x)
    p.gscale, p.gshift, p.gmean, p.grstd = _f32(gscale), _f32(gshift), _f32(gmean), _f32(grstd)
    p.tanh_out, p.stats_mode = int(tanh), stats_mode
    p.w_layout = int(kmajor)
    p.y_group = int(y_group)
    p.wsel, p.wsel_stride, p.order = _p(wsel), (need if wsel is not None else 0), _p(order)
    p.yperm, p.yperm_stride = None, 0
    if yperm is not None:
        if wsel is None or yperm.dtype != torch.int16 or yperm.dim() != 2 or yperm.shape[0] * need != wimg.numel() or not yperm.is_contiguous():
            raise _lib.McgenError('yperm must be a contiguous int16 [sets, stride] table that comes with wsel')
        p.yperm, p.yperm_stride = _p(yperm), yperm.shape[1]
    p.wlive = None
    if wlive is not None:
        if wsel is None or wlive.dtype != torch.int32 or not wlive.is_contiguous() or \
                tuple(wlive.shape) != (wimg.numel() // need, len(segs)) or wlive.device != wimg.device:
            raise _lib.McgenError('wlive must be a contiguous int32 [sets, segments] table that comes with wsel')
        p.wlive = _p(wlive)
    p.ycmap, p.ycmap_stride = None, 0
    if ycmap is not None:
        if ycmap.dtype != torch.int16 or tuple(ycmap.shape) != (n, cmap_stride(pad8(cout))):
            raise _lib.McgenError(f'ycmap must be int16 {(n, cmap_stride(pad8(cout)))}')
        p.ycmap, p.ycmap_stride = _p(ycmap), ycmap.shape[1]
    stats = None
    lib = _lib.load()
    plan = _conv_plan(p, dtype)          # one question per launch: rows of `stats`, the profile name, the test logs
    if stats_mode:
        stats = torch.empty((plan.m_tiles, 2, pad16(cout) if (ycmap is not None or yperm is not None) else cy), dtype=torch.float32, device=y.device)
        p.stats = _p(stats)
    kflops = 2.0 * n * h * w * cout * sum(s.ksize * s.ksize * s.x.shape[-1] for s in segs)

    def _name():
        base = f'conv_fused<{"bf16" if dtype == torch.bfloat16 else "f32"},{plan.bm},{plan.bn}{(",mc", ",gk")[kmajor - 1] if kmajor else ""}>'
        if plan.form:
            base = ('conv_skinny<bf16>', 'conv_smap<bf16>', 'conv_px1<bf16>', 'conv_c8<bf16>', 'conv_head<bf16>')[plan.form - 1]
        if _PROF_SHAPES:
            base += f' N{n} {h}x{w} ' + '+'.join(f'{s.x.shape[-1]}k{s.ksize}' for s in segs) + f'->{cout}' + \
                ('g' if gate_x is not None else '') + ('p' if pool else '') + (f's{stats_mode}' if stats_mode else '')
        return base
    if TILE_LOG is not None:
        bm, bn = C.c_int(plan.bm), C.c_int(plan.bn)
        if plan.form:       # a kernel in a file of its own has no tile: the log keeps naming the tile policy's pick
            check(lib.mcgen_conv_tile(C.byref(p), _dt(dtype), C.byref(bm), C.byref(bn)), 'conv_tile')
        TILE_LOG.append((bm.value, bn.value))
    if FORM_LOG is not None:
        FORM_LOG.append(kmajor)
    if KERNEL_LOG is not None:
        KERNEL_LOG.append(int(plan.form))
    _timed(_name, kflops, lambda: check(lib.mcgen_conv_fused(C.byref(p), _dt(dtype), _stream()), 'conv_fused'),
           lambda: _nbytes(wimg, y, res, gate_x, *[s.x for s in segs]))
    return y, stats


# ---- weight gradients: which kernel a layer gets, its pixel splits and the slab reductions ---------------
MULTI_LOG = None         # tools: receives (map side, ksize, 128-pixel steps, tiles, splits) per layer of every wgrad_multi launch
WGRAD_LOG = None         # tests: a list that receives which weight-gradient kernel family a call with default splits takes
BATCH_LOG = None         # tools / tests: receives the layer count of every mcgen_wgrad_batch launch
_deferred = None         # the open deferred_reduces context's queue (_ReduceJob and _PendingLayer entries, in call order)
_MULTI = _flag('MCGEN_WGRAD_MULTI', '1') != '0'        # eligible 3x3 weight gradients of a pass as one mcgen_wgrad_multi launch
_BATCH = _flag('MCGEN_WGRAD_BATCH', '1') != '0'        # the other layers of a pass: same-shape groups as one mcgen_wgrad_batch launch
_WG_GROUP_MIN = 1 << 30 if _flag('MCGEN_WGRAD_GROUP', '1') == '0' else 4      # chunks from which a 1x1 gradient runs as chunk groups
_WG_MAX_SPLITS = int(_flag('MCGEN_WGRAD_MAX_SPLITS', '128'))   # (64 left the thin image layers -- 2 blocks -- on half the chip)
_WG_TARGET = int(_flag('MCGEN_WGRAD_TARGET', '256'))   # workgroups a weight-gradient launch aims for
_WG_W1 = float(_flag('MCGEN_WG_W1', '0.55'))        # cost of a 1x1 layer's 128-pixel step relative to a 3x3 layer's (the same staging, a ninth of the MFMAs)
_WG_FIX = float(_flag('MCGEN_WG_FIX', '5'))        # fixed cost of a workgroup (setup, the accumulator flush) in steps
_CU_COUNT = {}


def _cu_count(device) -> int:
    n = _CU_COUNT.get(device)
    if n is None:
        n = _CU_COUNT[device] = torch.cuda.get_device_properties(device).multi_processor_count
    return n


def _default_splits(m_tiles: int, cout: int, nchunk: int, ksize: int, bf16: bool, h: int, w: int, n: int, c8: bool, paired: bool,
                    cus: int) -> int:
    """Pixel splits of a weight-gradient launch whose caller names none (`cus`: the device's CU count, read for c8 only)."""
    # 1x1 gradients with >= 4 chunks run as chunk groups of 4 (wgrad.hip): a quarter of the workgroups per split
    # (wgrad.hip: the ring form -- bf16, tiles inside one image -- comes first; chunk groups are for the small maps)
    ring = bf16 and h * w >= 128 and w <= 64 and (n * h * w) % 128 == 0
    grouped = ksize == 1 and nchunk >= _WG_GROUP_MIN and bf16 and not ring
    blocks = ((pad16(cout) + 63) // 64) * ((nchunk + 3) // 4 if grouped else nchunk)
    # enough workgroups to fill the chip matters more than the slab traffic (measured: 8x8 layers lose
    # 20 % with 16 instead of 64 splits)
    splits = max(1, min(m_tiles, (_WG_TARGET + blocks - 1) // blocks, _WG_MAX_SPLITS))
    if c8:
        # the image-layer kernel streams dy with every output channel in one workgroup (256-pixel steps): one per CU
        splits = max(1, min(m_tiles // 2, cus))
    if paired:
        splits = max(2, splits + (splits & 1))
    return splits


def _plan_multi(layers, budget: int):
    """Pixel splits of the layers of one mcgen_wgrad_multi launch: `layers` = [(m_tiles, blocks, ksize, side, paired)] (128-pixel
    steps, workgroup tiles per split, 1 or 3, map side, two-half launch), `budget` = workgroups the launch may total (one per CU).
    Pure integer / float arithmetic: tests/test_wgrad_plan_cpu.py pins it."""
    # Cost model of one workgroup of a layer with `sp` pixel splits: fix + (m_tiles / sp) * w in units of a 3x3
    # layer's 128-pixel step; the launch lasts as long as its slowest workgroup, so the splits are the smallest that
    # bring every layer under a common time T, T as small as the CU budget allows.  Calibrated with
    # tools/wgmulti_cost.py (one layer per launch, 16 .. 128 steps per workgroup): 3x3 4.0 us per step + 20 us fixed on
    # every map size (so `side` does not enter), 1x1 2.15 us per step + 6 us: w(1x1) = 0.55, fix = 5 steps (3x3) / 1.5 (1x1).
    # (The first version split in proportion to w * steps with w(1x1) = 0.35 and no fixed part: the generator's three
    # shortcut layers got one workgroup per tile and ran 256 steps each while the 3x3 layers' workgroups were done after
    # 86: 518 us for a pass that now takes 388; the discriminator's launches 143 -> 136 us.)
    rows = [(m_tiles, blocks, 1.0 if ksize == 3 else _WG_W1, _WG_FIX if ksize == 3 else 0.3 * _WG_FIX, 2 if paired else 1)
            for m_tiles, blocks, ksize, _side, paired in layers]

    def need(m_tiles, w, fix, unit, t):
        cap = max(unit, m_tiles // unit * unit)
        if t <= fix:
            return cap
        sp = int(-(-m_tiles * w // (t - fix)))
        sp = -(-sp // unit) * unit
        return max(unit, min(cap, sp))
    lo, hi = _WG_FIX, _WG_FIX + max(m_tiles * w for m_tiles, _, w, _, _ in rows) + 1.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if sum(need(m_tiles, w, fix, unit, mid) * blocks for m_tiles, blocks, w, fix, unit in rows) <= budget:
            hi = mid
        else:
            lo = mid
    splits = [need(m_tiles, w, fix, unit, hi) for m_tiles, _, w, fix, unit in rows]
    # hand the workgroups left over to the layers with the most work per workgroup
    used = sum(sp * r[1] for sp, r in zip(splits, rows))
    while True:
        best = None
        for i, (m_tiles, blocks, w, _, unit) in enumerate(rows):
            if splits[i] + unit <= m_tiles // unit * unit and used + unit * blocks <= budget:
                load = m_tiles / splits[i] * w
                if best is None or load > best[0]:
                    best = (load, i, unit, blocks)
        if best is None:
            return splits
        splits[best[1]] += best[2]
        used += best[2] * best[3]


class _ReduceJob(NamedTuple):
    """One slab reduction: the fields of mcgen_wreduce_t, as tensors where they are pointers (which keeps those alive)."""
    slabs: Tensor
    grad: Tensor
    bias_slabs: Optional[Tensor]
    bias_grad: Optional[Tensor]
    bias_grad2: Optional[Tensor]
    splits: int
    Cout: int
    Cin: int
    ksize: int
    Cout_w: int
    row_perm: int
    accumulate: int
    alpha: float
    row_scale: Optional[Tensor]
    cin_slab: int
    tapcols: int
    tap0: int
    ntap_out: int

    def fill(self, a: _lib.WReduce):
        """As one element of a mcgen_wgrad_reduce_batch table."""
        a.slabs, a.grad, a.bias_slabs = _p(self.slabs), _f32(self.grad), _p(self.bias_slabs)
        a.bias_grad = _f32(self.bias_grad) if self.bias_slabs is not None else None
        a.bias_grad2 = _f32(self.bias_grad2) if self.bias_slabs is not None else None
        a.splits, a.Cout, a.Cin, a.ksize, a.Cout_w = self.splits, self.Cout, self.Cin, self.ksize, self.Cout_w
        a.row_perm, a.accumulate, a.alpha = self.row_perm, self.accumulate, self.alpha
        a.row_scale, a.cin_slab = _f32(self.row_scale), self.cin_slab
        a.tapcols, a.tap0, a.ntap_out = self.tapcols, self.tap0, self.ntap_out

    def launch(self):
        """On its own, now (outside a deferred_reduces context)."""
        _timed(lambda: 'wgrad_reduce', 0.0,
               lambda: check(_lib.load().mcgen_wgrad_reduce(
                   _p(self.slabs), self.splits, _f32(self.grad), self.Cout, self.Cin, self.ksize, self.Cout_w, self.row_perm,
                   self.alpha, self.accumulate, _p(self.bias_slabs), _f32(self.bias_grad), _f32(self.bias_grad2), _f32(self.row_scale),
                   self.cin_slab, self.tapcols, self.tap0, self.ntap_out, _stream()), 'wgrad_reduce'),
               lambda: _nbytes(self.grad), lambda: _nbytes(self.slabs, self.bias_slabs))


class _PendingLayer:
    """One weight-gradient layer between ops.wgrad's checks and its slab reduction.  `kind`: 'multi' = queued for the pass's
    mcgen_wgrad_multi launch (`splits` comes from _plan_multi), 'batch' = queued for a same-shape mcgen_wgrad_batch launch,
    'single' = launched by ops.wgrad itself (never queued)."""
    __slots__ = ('kind', 'p', 'seg', 'dy', 'cout', 'cin', 'grad', 'bias_grad', 'bias_grad2', 'second', 'alpha', 'accumulate',
                 'row_perm', 'row_scale', 'taps', 'm_tiles', 'blocks', 'splits', 'c8', 'slabs', 'bias_slabs')

    def __init__(self, kind, p, seg, dy, cout, cin, grad, bias_grad, bias_grad2, second, alpha, accumulate, row_perm, row_scale, taps,
                 c8, m_tiles, blocks, splits):
        self.kind, self.p, self.seg, self.dy, self.cout, self.cin = kind, p, seg, dy, cout, cin
        self.grad, self.bias_grad, self.bias_grad2, self.second = grad, bias_grad, bias_grad2, second
        self.alpha, self.accumulate, self.row_perm, self.row_scale, self.taps = alpha, accumulate, row_perm, row_scale, taps
        self.m_tiles, self.blocks, self.splits, self.c8 = m_tiles, blocks, splits, c8
        self.slabs = self.bias_slabs = None

    def alloc(self):
        """Allocates the split-K slabs (and bias slabs) for `splits` and points the launch parameters at them; returns what
        _timed wants of the layer: (flops, algorithmic bytes, slab bytes)."""
        p, seg, ks, lib = self.p, self.seg, self.seg.ksize, _lib.load()
        elems = int(lib.mcgen_wgrad_c8_slab_elems(C.byref(p)) if self.c8 else lib.mcgen_wgrad_slab_elems(C.byref(p)))
        self.slabs = torch.empty((self.splits, elems), dtype=torch.float32, device=self.dy.device)
        if self.bias_grad is not None:
            self.bias_slabs = torch.empty((self.splits * 4, pad16(self.cout)), dtype=torch.float32, device=self.dy.device)
        p.splits, p.slabs, p.bias_slabs = self.splits, _p(self.slabs), _p(self.bias_slabs)
        # algorithmic bytes: x + dy read once, dW (+ db) written once; the split-K slabs are the implementation's
        return (2.0 * p.N * p.H * p.W * self.cout * seg.x.shape[-1] * ks ** 2,
                _nbytes(seg.x, self.dy) + 4 * (self.cout * self.cin * ks ** 2 + (self.cout if self.bias_grad is not None else 0)) * (2 if self.second is not None else 1),
                _nbytes(self.slabs, self.bias_slabs))

    def jobs(self):
        """The layer's slab reduction(s): one, or one per half of a two-half launch, each over its half of the slabs."""
        tail = (self.cout, self.cin, self.seg.ksize, pad16(self.cout), self.row_perm, int(self.accumulate), float(self.alpha),
                self.row_scale, self.seg.x.shape[-1], int(self.c8)) + tuple(self.taps)
        if self.second is None:
            return [_ReduceJob(self.slabs, self.grad, self.bias_slabs, self.bias_grad, self.bias_grad2, self.splits, *tail)]
        hs = self.splits // 2
        b0, b1 = (self.bias_slabs[:hs * 4], self.bias_slabs[hs * 4:]) if self.bias_slabs is not None else (None, None)
        return [_ReduceJob(self.slabs[:hs], self.grad, b0, self.bias_grad, self.bias_grad2, hs, *tail),
                _ReduceJob(self.slabs[hs:], self.second[0], b1, self.second[1], self.second[2], hs, *tail)]


def _alloc_table(grp):
    """alloc() for every layer of one multi / batch launch -> (the launch's mcgen_wgrad_t table, flops, bytes, slab bytes)."""
    arr = (_lib.Wgrad * len(grp))()
    flops = nbytes = extra = 0.0
    for a, q in zip(arr, grp):
        f, b, e = q.alloc()
        flops, nbytes, extra = flops + f, nbytes + b, extra + e
        C.memmove(C.byref(a), C.byref(q.p), C.sizeof(_lib.Wgrad))
    return arr, flops, nbytes, extra


def wgrad(seg: Seg, dy: Tensor, cout: int, cin: int, grad: Tensor, *, dy_ups: bool = False,
          alpha: float = 1.0, accumulate: bool = False, row_perm: int = 1, splits: Optional[int] = None,
          bias_grad: Optional[Tensor] = None, bias_grad2: Optional[Tensor] = None, second=None,
          row_scale: Optional[Tensor] = None, taps: Optional[Tuple[int, int]] = None):
    """grad[Cout, Cin, k, k] (+)= alpha * dW of one fused-conv segment; optionally also the bias
    gradient bias_grad[Cout] (+)= alpha * sum_pixels dy (and a copy into bias_grad2).
    `cin` may be smaller than the (padded) channel count of seg.x: only the first cin input channels are written.
    `row_scale[Cout]` (optional) multiplies row co of the weight gradient and entry co of the bias gradients.
    `second` = (grad_b, bias_grad_b, bias_grad2_b): the batch is two halves (paired discriminator pass) and the
    second half's gradient goes to these tensors instead -- one launch, one slab set per half.
    `taps` = (tap0, n): grad is [Cout, Cin, n] and receives taps tap0 .. tap0 + n - 1 of the k x k gradient only (a sub-kernel
    embedded in the 3x3 image: MCGatedMaskedConv2d's (2 x 3) / (1 x 2) stacks) -- no scratch tensor + slice copy."""
    n = seg.x.shape[0]
    h = seg.x.shape[1] * (2 if seg.ups else 1)
    w = seg.x.shape[2] * (2 if seg.ups else 1)
    dtype = seg.x.dtype
    p = _lib.Wgrad()
    seg.fill(p.seg)
    p.dy = _p(dy)
    p.N, p.H, p.W = n, h, w
    p.Cout, p.Cout_w, p.Cdy = cout, pad16(cout), dy.shape[-1]
    p.dy_ups = int(dy_ups)
    exp = (n, h // 2, w // 2) if dy_ups else (n, h, w)
    if tuple(dy.shape[:3]) != exp or dy.dtype != dtype:
        raise _lib.McgenError(f'dy must be {exp}+[C] {dtype}, got {tuple(dy.shape)} {dy.dtype}')
    m_tiles = (n * h * w + 127) // 128
    explicit_splits = splits
    # the image-side layers (conv input = the 8-channel image tensor) have their own kernel and compact slabs (wgrad_c8.hip)
    c8 = bool(_lib.load().mcgen_wgrad_c8_ok(C.byref(p), _dt(dtype)))
    if WGRAD_LOG is not None:
        WGRAD_LOG.append('c8' if c8 else 'general')
    if splits is None:
        splits = _default_splits(m_tiles, cout, (seg.x.shape[-1] + 31) // 32, seg.ksize, dtype == torch.bfloat16, h, w, n, c8,
                                 second is not None, _cu_count(dy.device) if c8 else 0)
    if second is not None and ((n * h * w) % 256 != 0 or splits % 2):
        raise _lib.McgenError('wgrad: a two-half launch needs whole 128-pixel tiles per half and even splits')
    p.splits = splits
    p.halves = int(second is not None)
    lib = _lib.load()
    tap0, ntap_out = taps if taps is not None else (0, 0)
    if taps is not None and (second is not None or not (0 <= tap0 and 0 < ntap_out and tap0 + ntap_out <= seg.ksize ** 2)):
        raise _lib.McgenError('wgrad: bad tap window (and tap windows do not combine with two-half launches)')
    if grad.numel() != cout * cin * (ntap_out or seg.ksize * seg.ksize):
        raise _lib.McgenError(f'grad has {grad.numel()} elements, expected {cout * cin * (ntap_out or seg.ksize ** 2)}')
    kind, blocks = 'single', 0
    if (_deferred is not None and _MULTI and explicit_splits is None and dtype == torch.bfloat16
            and lib.mcgen_wgrad_multi_ok(C.byref(p), _dt(dtype))):
        # The 3x3 layers of a backward pass share ONE launch (mcgen_wgrad_multi): queued here, launched when the pass's
        # deferred_reduces context closes -- its pixel splits are sized by the layer's share of the pass's FLOPs.
        kind, blocks, splits = 'multi', (pad16(cout) // 128) * (seg.x.shape[-1] // 64), None
    elif (_deferred is not None and _BATCH and dtype == torch.bfloat16 and not c8 and second is None and explicit_splits is None
            and splits * _lib.WGRAD_MULTI_MAX <= 65535):
        # Layers the pass-wide kernel does not take (skinny channel counts, 4x4 maps ...) wait for the end of the pass too: those of
        # IDENTICAL shape share one launch of their kernel (mcgen_wgrad_batch: MCGlow has 16 flows per level)
        kind = 'batch'
    q = _PendingLayer(kind, p, seg, dy, cout, cin, grad, bias_grad, bias_grad2, second, alpha, accumulate, row_perm, row_scale,
                      (tap0, ntap_out), c8, m_tiles, blocks, splits)
    if kind != 'single':
        if not grad.is_contiguous():
            raise _lib.McgenError('deferred wgrad reduce needs a contiguous gradient tensor')
        _deferred.append(q)
        return
    flops, nbytes, extra = q.alloc()
    _timed(lambda: f'wgrad<{"bf16" if dtype == torch.bfloat16 else "f32"},{seg.ksize}>' + (
        f' N{n} {h}x{w} {seg.x.shape[-1]}->{cout} s{splits}' if _PROF_SHAPES else ''), flops,
           lambda: check(lib.mcgen_wgrad(C.byref(p), _dt(dtype), _stream()), 'wgrad'), lambda: nbytes, lambda: extra)
    for job in q.jobs():
        if _deferred is None:
            job.launch()
        elif not job.grad.is_contiguous():
            raise _lib.McgenError('deferred wgrad reduce needs a contiguous gradient tensor')
        else:
            _deferred.append(job)


def _launch_multi(pend):
    """Size the queued layers' pixel splits by their share of the pass's work (_plan_multi: one workgroup per CU over the
    whole launch), allocate the slabs and launch mcgen_wgrad_multi (<= MCGEN_WGRAD_MULTI_MAX layers each)."""
    lib = _lib.load()
    budget = _cu_count(pend[0].dy.device)
    for base in range(0, len(pend), _lib.WGRAD_MULTI_MAX):
        grp = pend[base:base + _lib.WGRAD_MULTI_MAX]
        plan = _plan_multi([(q.m_tiles, q.blocks, q.seg.ksize, q.p.H, q.second is not None) for q in grp], budget)
        for q, sp in zip(grp, plan):
            q.splits = sp
        if MULTI_LOG is not None:
            MULTI_LOG.append([(q.p.H, q.seg.ksize, q.m_tiles, q.blocks, q.splits) for q in grp])
        arr, flops, nbytes, extra = _alloc_table(grp)
        _timed(lambda: 'wgrad_multi<bf16>', flops,
               lambda: check(lib.mcgen_wgrad_multi(arr, len(grp), _lib.BF16, _stream()), 'wgrad_multi'),
               lambda: nbytes, lambda: extra)


def _launch_batches(pend):
    """Queued layers outside mcgen_wgrad_multi: groups of identical shape as one mcgen_wgrad_batch launch each (<= MCGEN_WGRAD_MULTI_MAX
    layers), the rest one by one; slabs allocated here, the reduce jobs follow with the pass's batched reduce."""
    lib = _lib.load()
    groups = {}
    for q in pend:
        p = q.p
        key = (p.N, p.H, p.W, p.Cout, p.Cout_w, p.Cdy, p.dy_ups, p.splits, p.seg.C, p.seg.ksize, p.seg.ups, q.bias_grad is not None)
        groups.setdefault(key, []).append(q)
    for grp_all in groups.values():
        for base in range(0, len(grp_all), _lib.WGRAD_MULTI_MAX):
            grp = grp_all[base:base + _lib.WGRAD_MULTI_MAX]
            arr, flops, nbytes, extra = _alloc_table(grp)
            ks = grp[0].seg.ksize
            if BATCH_LOG is not None:
                BATCH_LOG.append(len(grp))
            _timed(lambda: f'wgrad<bf16,{ks}>', flops,
                   lambda: (check(lib.mcgen_wgrad(C.byref(grp[0].p), _lib.BF16, _stream()), 'wgrad') if len(grp) == 1 else
                            check(lib.mcgen_wgrad_batch(arr, len(grp), _lib.BF16, _stream()), 'wgrad_batch')),
                   lambda: nbytes, lambda: extra)


class deferred_reduces:
    """Within this context every ops.wgrad launches only its split-K kernel; the slab reductions of the whole pass
    run as ONE table-driven launch on exit (a backward pass has ~10 of them, each too small to fill the chip)."""

    def __enter__(self):
        global _deferred
        self._outer = _deferred
        _deferred = []
        return self

    def __exit__(self, et, ev, tb):
        global _deferred
        queue, _deferred = _deferred, self._outer
        if et is not None or not queue:
            return False
        kinds = {'multi': [], 'batch': []}
        for q in queue:
            if isinstance(q, _PendingLayer):
                kinds[q.kind].append(q)
        if kinds['batch']:
            _launch_batches(kinds['batch'])
        if kinds['multi']:
            _launch_multi(kinds['multi'])
        jobs = [j for q in queue for j in (q.jobs() if isinstance(q, _PendingLayer) else (q,))]
        arr = (_lib.WReduce * len(jobs))()
        for a, j in zip(arr, jobs):
            j.fill(a)
        _timed(lambda: 'wgrad_reduce', 0.0,
               lambda: check(_lib.load().mcgen_wgrad_reduce_batch(arr, len(jobs), _stream()), 'wgrad_reduce_batch'),
               lambda: sum(_nbytes(j.grad) for j in jobs), lambda: sum(_nbytes(j.slabs, j.bias_slabs) for j in jobs))
        return False


def bn_finalize(partials: Tensor, count: int, gamma: Tensor, beta: Tensor,
                running_mean: Optional[Tensor], running_var: Optional[Tensor],
                momentum: float = 0.1, eps: float = 1e-5, fold: int = 1, groups: int = 1):
    """-> (scale, shift, mean, rstd), each [C] ([groups, C] for groups > 1: `count` is per group and the running stats
    take the groups' momentum updates in order); running stats updated in place."""
    tiles, _, pitch = partials.shape
    c = gamma.numel()
    out = torch.empty((4, groups, c), dtype=torch.float32, device=partials.device)
    check(_lib.load().mcgen_bn_finalize_groups(_f32(partials), tiles, pitch, fold, c, float(count), groups, _f32(gamma), _f32(beta),
                                               _f32(running_mean), _f32(running_var), momentum, eps,
                                               out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                               _stream()), 'bn_finalize')
    if groups == 1:
        out = out.view(4, c)
    return out[0], out[1], out[2], out[3]


def bn_finalize_batch(items):
    """items = [(partials, count, gamma, beta, running_mean, running_var, momentum, eps)]: several independent BatchNorm layers
    finalized in ONE launch (mcgen_bn_finalize_batch, <= 4) -> [(scale, shift, mean, rstd)] as bn_finalize gives per layer."""
    arr = (_lib.BnFin * len(items))()
    outs = []
    for d, (partials, count, gamma, beta, rm, rv, momentum, eps) in zip(arr, items):
        tiles, _, pitch = partials.shape
        c = gamma.numel()
        out = torch.empty((4, c), dtype=torch.float32, device=partials.device)
        d.partials, d.tiles, d.pitch, d.fold, d.C, d.count = _f32(partials), tiles, pitch, 1, c, float(count)
        d.gamma, d.beta, d.running_mean, d.running_var = _f32(gamma), _f32(beta), _f32(rm), _f32(rv)
        d.momentum, d.eps = float(momentum), float(eps)
        d.scale, d.shift, d.mean, d.rstd = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr()
        outs.append((out[0], out[1], out[2], out[3]))
    check(_lib.load().mcgen_bn_finalize_batch(arr, len(items), _stream()), 'bn_finalize_batch')
    return outs


def bn_finalize_par(partials: Tensor, count: int, gamma: Tensor, beta: Tensor, eps: float = 1e-5, fold: int = 1, groups: int = 1):
    """bn_finalize with the statistics groups in parallel and the running statistics left alone
    -> (scale, shift, mean, rstd, unbiased var), each [groups, C]; pair with bn_running_batch at the end of the pass."""
    tiles, _, pitch = partials.shape
    c = gamma.numel()
    out = torch.empty((5, groups, c), dtype=torch.float32, device=partials.device)
    check(_lib.load().mcgen_bn_finalize_par(_f32(partials), tiles, pitch, fold, c, float(count), groups, _f32(gamma), _f32(beta), eps,
                                            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(),
                                            _stream()), 'bn_finalize_par')
    return out[0], out[1], out[2], out[3], out[4]


def bn_running_batch(items):
    """items = [(running_mean, running_var, mean [groups, C], unb [groups, C], momentum)]: every layer's running statistics
    take its groups' updates in order, one launch (mcgen_bn_running_batch)."""
    arr = (_lib.BnRun * len(items))()
    for d, (rm, rv, mean, unb, mom) in zip(arr, items):
        d.running_mean, d.running_var, d.mean, d.unb = _f32(rm), _f32(rv), _f32(mean), _f32(unb)
        d.groups, d.C, d.momentum = mean.shape[0], rm.numel(), float(mom)
    check(_lib.load().mcgen_bn_running_batch(arr, len(items), _stream()), 'bn_running_batch')


def bn_eval_affine(gamma, beta, running_mean, running_var, eps: float = 1e-5):
    c = gamma.numel()
    out = torch.empty((2, c), dtype=torch.float32, device=gamma.device)
    check(_lib.load().mcgen_bn_eval_affine(_f32(gamma), _f32(beta), _f32(running_mean), _f32(running_var), eps, c,
                                           out[0].data_ptr(), out[1].data_ptr(), _stream()), 'bn_eval_affine')
    return out[0], out[1]


def bn_backward(partials: Tensor, dz: Tensor, x: Tensor, count: int, scale, mean, rstd,
                dgamma: Optional[Tensor], dbeta: Optional[Tensor], add: Optional[Tensor] = None,
                accumulate: bool = False) -> Tensor:
    """BN backward from the conv epilogue's (sum dz, sum dz*xhat) partials."""
    tiles, _, pitch = partials.shape
    c = scale.numel()
    sums = torch.empty((2, c), dtype=torch.float32, device=dz.device)
    lib = _lib.load()
    check(lib.mcgen_bn_bwd_finalize(_f32(partials), tiles, pitch, c, _f32(dgamma), _f32(dbeta), _f32(sums),
                                    int(accumulate), _stream()), 'bn_bwd_finalize')
    dx = torch.empty_like(dz)
    assert dz.shape[-1] == c and x.shape == dz.shape
    check(lib.mcgen_bn_bwd_apply(_p(dz), _p(x), _p(add), _p(dx), _dt(dz.dtype), dz.numel() // c, c, _f32(sums),
                                 float(count), _f32(scale), _f32(mean), _f32(rstd), _stream()), 'bn_bwd_apply')
    return dx


_colsum_ws = {}


def colsum(x: Tensor, c: int, out: Tensor, alpha: float = 1.0, accumulate: bool = False, row_perm: int = 1):
    """out[c] (+)= alpha * sum over all leading dims of x[..., :c]."""
    pitch = x.shape[-1]
    rows = x.numel() // pitch
    ws = torch.empty(256 * c, dtype=torch.float32, device=x.device)
    check(_lib.load().mcgen_colsum(_p(x), _dt(x.dtype), rows, c, pitch, _f32(out), row_perm, float(alpha),
                                   int(accumulate), _f32(ws), _stream()), 'colsum')


def tanh_bwd(dy: Tensor, y: Tensor) -> Tensor:
    dx = torch.empty_like(dy)
    check(_lib.load().mcgen_tanh_bwd(_p(dy), _p(y), _p(dx), _dt(dy.dtype), dy.numel(), _stream()), 'tanh_bwd')
    return dx


def dtail_fwd(x: Tensor, code: Optional[Tensor], w: Tensor, b: Tensor, sigma: Tensor):
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    pooled = torch.empty((n, c), dtype=torch.float32, device=x.device)
    logit = torch.empty((n,), dtype=torch.float32, device=x.device)
    check(_lib.load().mcgen_dtail_fwd(_p(x), _dt(x.dtype), _f32(code), _f32(w), _f32(b), _f32(sigma), _f32(pooled),
                                      _f32(logit), n, hw, c, _stream()), 'dtail_fwd')
    return logit, pooled


def dtail_bwd(dlogit: Tensor, x: Tensor, code, w, sigma, pooled, dw: Optional[Tensor], db: Optional[Tensor],
              accumulate: bool = False) -> Tensor:
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    dx = torch.empty_like(x)
    check(_lib.load().mcgen_dtail_bwd(_f32(dlogit), _p(x), _dt(x.dtype), _f32(code), _f32(w), _f32(sigma), _f32(pooled),
                                      _p(dx), _f32(dw), _f32(db), n, hw, c, int(accumulate), _stream()), 'dtail_bwd')
    return dx


def dtail_hinge_ok(x: Tensor) -> bool:
    c = x.shape[-1]
    return c % 8 == 0 and c <= 2048


def dtail_hinge_fused(x: Tensor, code: Optional[Tensor], w: Tensor, b: Tensor, sigma: Tensor, mode: str):
    """Tail forward + d(hinge loss)/d(logit) + tail input gradient in one launch (mcgen_dtail_hinge_fused).
    mode 'd_pair': x is a paired batch (real half, generated half), hinge_d; 'g': hinge_g.
    -> (logit [N], pooled [N, C], dlogit [N], dx like x)"""
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    pooled = torch.empty((n, c), dtype=torch.float32, device=x.device)
    both = torch.empty((2, n), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    check(_lib.load().mcgen_dtail_hinge_fused(_p(x), _dt(x.dtype), _f32(code), _f32(w), _f32(b), _f32(sigma), _f32(pooled),
                                              both[0].data_ptr(), both[1].data_ptr(), _p(dx), n, hw, c,
                                              {'d_pair': 0, 'g': 1}[mode], _stream()), 'dtail_hinge_fused')
    return both[0], pooled, both[1], dx


def gan_loss_id(loss_type: str) -> int:
    """cfg['loss_type'] (train_gan.py:55) -> MCGEN_GAN_LOSS_*; anything else is the reference's error (train_gan.py:156)."""
    if loss_type not in ('Hinge', 'BCE'):
        raise ValueError('Not valid loss type')
    return _lib.CONSTANTS['MCGEN_GAN_LOSS_HINGE' if loss_type == 'Hinge' else 'MCGEN_GAN_LOSS_BCE']


def dtail_loss_fused(x: Tensor, code: Optional[Tensor], w: Tensor, b: Tensor, sigma: Tensor, mode: str, loss_type: str):
    """`dtail_hinge_fused` with the loss chosen (mcgen_dtail_loss_fused): 'Hinge' gives its bits, 'BCE' forms
    d(binary_cross_entropy_with_logits)/d(logit) of train_gan.py:149-152 ('d_pair') / 169-170 ('g') from the sample's logit.
    -> (logit [N], pooled [N, C], dlogit [N], dx like x)"""
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    pooled = torch.empty((n, c), dtype=torch.float32, device=x.device)
    both = torch.empty((2, n), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    check(_lib.load().mcgen_dtail_loss_fused(_p(x), _dt(x.dtype), _f32(code), _f32(w), _f32(b), _f32(sigma), _f32(pooled),
                                             both[0].data_ptr(), both[1].data_ptr(), _p(dx), n, hw, c,
                                             {'d_pair': 0, 'g': 1}[mode], gan_loss_id(loss_type), _stream()), 'dtail_loss_fused')
    return both[0], pooled, both[1], dx


def lecam_state_layout():
    """mcgen_lecam_state_t as a tensor: -> (int64 words of the struct, {float field: float32 index}, int64 index of t),
    read off the header's struct, so that a holder keeps the state as ONE int64 tensor with float32 / int64 views."""
    st = _lib.LecamState
    floats = {k: getattr(st, k).offset // 4 for k in ('a_real', 'a_fake', 'm_real', 'm_fake', 'r_t', 'reg')}
    return C.sizeof(st) // 8, floats, st.t.offset // 8


def _lecam_state(state: Tensor) -> int:
    """The device address of a mcgen_lecam_state_t held as an int64 tensor (`lecam_state_layout`)."""
    if state is None or state.dtype != torch.int64 or state.numel() * 8 != C.sizeof(_lib.LecamState):
        raise _lib.McgenError('LeCam state: an int64 device tensor of sizeof(mcgen_lecam_state_t) bytes')
    return _p(state)


def dtail_lecam_fused(x: Tensor, code: Optional[Tensor], w: Tensor, b: Tensor, sigma: Tensor, loss_type: str,
                      state: Tensor, lam: float, start: int):
    """`dtail_loss_fused`, mode 'd_pair', with the LeCam regulariser's term in dlogit (mcgen_dtail_lecam_fused): the launch
    reads the anchors and the update count from `state` and leaves them alone -- `dtail_pair_wgrad(..., lecam=...)` of the
    same update writes them.  -> (logit [N], pooled [N, C], dlogit [N], dx like x)"""
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    pooled = torch.empty((n, c), dtype=torch.float32, device=x.device)
    both = torch.empty((2, n), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    check(_lib.load().mcgen_dtail_lecam_fused(_p(x), _dt(x.dtype), _f32(code), _f32(w), _f32(b), _f32(sigma), _f32(pooled),
                                              both[0].data_ptr(), both[1].data_ptr(), _p(dx), n, hw, c, gan_loss_id(loss_type),
                                              _lecam_state(state), float(lam), int(start), _stream()), 'dtail_lecam_fused')
    return both[0], pooled, both[1], dx


def lecam_loss_d(real: Tensor, fake: Tensor, loss_type: str, state: Tensor, lam: float, decay: float, start: int,
                 both: bool = False):
    """`gan_loss_d` with the LeCam regulariser (mcgen_lecam_loss_d): (loss, d loss / d real, d loss / d fake) from the
    anchors as `state` holds them, then the launch moves the anchors, writes the update's statistics and counts the update."""
    n = real.numel()
    out = torch.empty(1 + 2 * n, dtype=torch.float32, device=real.device)
    check(_lib.load().mcgen_lecam_loss_d(_f32(real), _f32(fake), n, gan_loss_id(loss_type), _lecam_state(state), float(lam),
                                         float(decay), int(start), out.data_ptr(), out[1:1 + n].data_ptr(), out[1 + n:].data_ptr(),
                                         _stream()), 'lecam_loss_d')
    if both:
        return out[0], out[1:1 + n], out[1 + n:], out[1:]
    return out[0], out[1:1 + n], out[1 + n:]


def dtail_pair_wgrad(dlogit: Tensor, pooled: Tensor, ratio: Tensor, dw1: Tensor, db1: Tensor, dw2: Tensor, db2: Tensor,
                     logit: Optional[Tensor] = None, loss: Optional[Tensor] = None, loss_type: str = 'Hinge', lecam=None):
    """Tail weight / bias gradients of the two halves of a paired discriminator pass (dw2 divided by ratio[0]); with
    `logit` [2N] and `loss` [1] the launch also writes the discriminator's loss of `loss_type` (train_gan.py:148-154).
    `lecam` = (state, lambda, decay, start): the loss value includes the LeCam regulariser and the launch updates `state`
    (mcgen_dtail_pair_wgrad_lecam_loss); it needs `logit` and `loss`."""
    n2, c = pooled.shape
    for t in (dw1, db1, dw2, db2):
        if not t.is_contiguous() or t.dtype != torch.float32:
            raise _lib.McgenError('dtail_pair_wgrad: outputs must be contiguous fp32')
    if lecam is not None:
        if loss is None or logit is None:
            raise _lib.McgenError('dtail_pair_wgrad: the LeCam state is updated by the launch that writes the loss value')
        state, lam, decay, start = lecam
        check(_lib.load().mcgen_dtail_pair_wgrad_lecam_loss(_f32(dlogit), _f32(pooled), _f32(ratio), _f32(logit.contiguous()), n2 // 2, c,
                                                            _f32(dw1), _f32(db1), _f32(dw2), _f32(db2), _f32(loss),
                                                            gan_loss_id(loss_type), _lecam_state(state), float(lam), float(decay),
                                                            int(start), _stream()), 'dtail_pair_wgrad_lecam_loss')
        return
    if loss is not None:
        check(_lib.load().mcgen_dtail_pair_wgrad_gan_loss(_f32(dlogit), _f32(pooled), _f32(ratio), _f32(logit.contiguous()), n2 // 2, c,
                                                          _f32(dw1), _f32(db1), _f32(dw2), _f32(db2), _f32(loss),
                                                          gan_loss_id(loss_type), _stream()), 'dtail_pair_wgrad_gan_loss')
        return
    check(_lib.load().mcgen_dtail_pair_wgrad(_f32(dlogit), _f32(pooled), _f32(ratio), n2 // 2, c,
                                             _f32(dw1), _f32(db1), _f32(dw2), _f32(db2), _stream()), 'dtail_pair_wgrad')


def hinge_d(real: Tensor, fake: Tensor, both: bool = False):
    """(loss, d loss / d real, d loss / d fake) of the discriminator hinge loss; `both`: also the two gradients as one
    contiguous [2N] tensor (they are views of it)."""
    n = real.numel()
    out = torch.empty(1 + 2 * n, dtype=torch.float32, device=real.device)
    check(_lib.load().mcgen_hinge_d(_f32(real), _f32(fake), n, out.data_ptr(), out[1:1 + n].data_ptr(),
                                    out[1 + n:].data_ptr(), _stream()), 'hinge_d')
    if both:
        return out[0], out[1:1 + n], out[1 + n:], out[1:]
    return out[0], out[1:1 + n], out[1 + n:]


def hinge_g(fake: Tensor):
    n = fake.numel()
    out = torch.empty(1 + n, dtype=torch.float32, device=fake.device)
    check(_lib.load().mcgen_hinge_g(_f32(fake), n, out.data_ptr(), out[1:].data_ptr(), _stream()), 'hinge_g')
    return out[0], out[1:]


def gan_loss_d(real: Tensor, fake: Tensor, loss_type: str, both: bool = False):
    """`hinge_d` with the loss chosen ('Hinge' | 'BCE', train_gan.py:148-154): (loss, d loss / d real, d loss / d fake),
    `both`: also the two gradients as one contiguous [2N] tensor."""
    n = real.numel()
    out = torch.empty(1 + 2 * n, dtype=torch.float32, device=real.device)
    check(_lib.load().mcgen_gan_loss_d(_f32(real), _f32(fake), n, gan_loss_id(loss_type), out.data_ptr(),
                                       out[1:1 + n].data_ptr(), out[1 + n:].data_ptr(), _stream()), 'gan_loss_d')
    if both:
        return out[0], out[1:1 + n], out[1 + n:], out[1:]
    return out[0], out[1:1 + n], out[1 + n:]


def gan_loss_g(fake: Tensor, loss_type: str):
    """`hinge_g` with the loss chosen (train_gan.py:168-172): (loss, d loss / d fake)."""
    n = fake.numel()
    out = torch.empty(1 + n, dtype=torch.float32, device=fake.device)
    check(_lib.load().mcgen_gan_loss_g(_f32(fake), n, gan_loss_id(loss_type), out.data_ptr(), out[1:].data_ptr(), _stream()),
          'gan_loss_g')
    return out[0], out[1:]


def sn_layers_tensor(layers, device) -> Tensor:
    """Pack [(w_off, u_off, v_off, rows, cols)] into a device byte tensor of mcgen_sn_layer_t."""
    arr = (_lib.SnLayer * len(layers))()
    for i, (wo, uo, vo, r, c) in enumerate(layers):
        arr[i].w_off, arr[i].u_off, arr[i].v_off, arr[i].rows, arr[i].cols = wo, uo, vo, r, c
    raw = bytes(arr)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def sn_power_iter(w_base: Tensor, uv_base: Tensor, layers_dev: Tensor, nlayers: int, do_iter: bool, sigma: Tensor,
                  max_rows: int, max_cols: int, snap: Optional[Tensor] = None):
    """`snap` (training mode): a buffer shaped like uv_base that receives the new u, v as well (the forward's own copy)."""
    ws = torch.empty(nlayers * (32 * max_cols + max_rows), dtype=torch.float32, device=w_base.device)
    if snap is not None:
        if not do_iter or snap.numel() != uv_base.numel() or snap.dtype != torch.float32:
            raise _lib.McgenError('sn_power_iter: snap needs a training-mode iteration and a float32 buffer like uv_base')
        check(_lib.load().mcgen_sn_power_iter_snap(_f32(w_base), _f32(uv_base), _p(layers_dev), nlayers, _f32(sigma), _f32(ws),
                                                   max_rows, max_cols, _f32(snap), _stream()), 'sn_power_iter_snap')
        return
    check(_lib.load().mcgen_sn_power_iter(_f32(w_base), _f32(uv_base), _p(layers_dev), nlayers, int(do_iter),
                                          _f32(sigma), _f32(ws), max_rows, max_cols, _stream()), 'sn_power_iter')


def sn_power_iter_rounds(w_base: Tensor, uv_base: Tensor, layers_dev: Tensor, nlayers: int, rounds: int,
                         max_rows: int, max_cols: int, snapshot: bool = True):
    """`rounds` training-mode power iterations in 2 * rounds + 1 launches (mcgen_sn_power_iter_rounds)
    -> (sigma [rounds + 1, nlayers], u/v snapshots [rounds, uv] or None); for rounds >= 2 the extra last row of `sigma` is
    sigma[rounds - 2] / sigma[rounds - 1] (the ratio a paired pass scales its second half by)."""
    sigma = torch.empty((rounds + 1, nlayers), dtype=torch.float32, device=w_base.device)
    snap = torch.empty((rounds, uv_base.numel()), dtype=torch.float32, device=w_base.device) if snapshot else None
    ws = torch.empty(nlayers * (32 * max_cols + max_rows), dtype=torch.float32, device=w_base.device)
    check(_lib.load().mcgen_sn_power_iter_rounds(_f32(w_base), _f32(uv_base), _p(layers_dev), nlayers, rounds, _f32(sigma), _f32(ws),
                                                 max_rows, max_cols, _f32(snap), uv_base.numel(), sigma[rounds].data_ptr(), _stream()),
          'sn_power_iter_rounds')
    return sigma, snap


def sn_power_iter_fused(w_base: Tensor, uv_base: Tensor, layers_dev: Tensor, nlayers: int, rounds: int, do_iter: bool,
                        max_rows: int, max_cols: int, snapshot: bool = True):
    """`rounds` power iterations of all layers in one launch -> (sigma [rounds, nlayers], u/v snapshots [rounds, uv] or None)."""
    sigma = torch.empty((rounds, nlayers), dtype=torch.float32, device=w_base.device)
    snap = torch.empty((rounds, uv_base.numel()), dtype=torch.float32, device=w_base.device) if snapshot else None
    check(_lib.load().mcgen_sn_power_iter_fused(_f32(w_base), _f32(uv_base), _p(layers_dev), nlayers, rounds, int(do_iter),
                                                _f32(sigma), _f32(snap), uv_base.numel(), max_rows, max_cols, _stream()),
          'sn_power_iter_fused')
    return sigma, snap


def sn_grad_fix(g_src: Tensor, g_dst: Tensor, w_base: Tensor, uv_base: Tensor, layers_dev: Tensor, nlayers: int,
                sigma: Tensor, accumulate: bool = False):
    ws = torch.empty(32 * nlayers, dtype=torch.float32, device=g_src.device)
    check(_lib.load().mcgen_sn_grad_fix(_f32(g_src), _f32(g_dst), _f32(w_base), _f32(uv_base), _p(layers_dev), nlayers,
                                        _f32(sigma), int(accumulate), _f32(ws), _stream()), 'sn_grad_fix')


def sn_grad_fix_pair(g_src0: Tensor, g_src1: Tensor, g_dst: Tensor, w_base: Tensor, uv0: Tensor, uv1: Tensor,
                     layers_dev: Tensor, nlayers: int, sigma0: Tensor, sigma1: Tensor, accumulate: bool = False):
    """Both halves of a paired discriminator pass in one dot + one apply launch (mcgen_sn_grad_fix_pair)."""
    ws = torch.empty(2 * 32 * nlayers, dtype=torch.float32, device=g_dst.device)
    check(_lib.load().mcgen_sn_grad_fix_pair(_f32(g_src0), _f32(g_src1), _f32(g_dst), _f32(w_base), _f32(uv0), _f32(uv1),
                                             _p(layers_dev), nlayers, _f32(sigma0), _f32(sigma1), int(accumulate), _f32(ws),
                                             _stream()), 'sn_grad_fix_pair')


def sn_fix_pair_adam(g_src0: Tensor, g_src1: Tensor, p: Tensor, m: Tensor, v: Tensor, uv0: Tensor, uv1: Tensor,
                     layers_dev: Tensor, nlayers: int, sigma0: Tensor, sigma1: Tensor, step: Tensor, lr, betas,
                     eps: float, weight_decay: float, advance_step: bool):
    """mcgen_sn_fix_pair_adam: the spectral-norm gradient fix of both halves of a paired discriminator pass fused with
    Adam's update of the same layers (`step`: the int64[2] {counter, ticket} buffer of ops.adam; `lr` as in ops.adam)."""
    assert step.dtype == torch.int64 and step.numel() == 2
    ws = torch.empty(2 * 32 * nlayers, dtype=torch.float32, device=p.device)
    lr_f, lr_dev = _lr_args(lr)
    check(_lib.load().mcgen_sn_fix_pair_adam(_f32(g_src0), _f32(g_src1), _f32(p), _f32(m), _f32(v), _f32(uv0), _f32(uv1),
                                             _p(layers_dev), nlayers, _f32(sigma0), _f32(sigma1), _f32(ws), lr_f, lr_dev, betas[0], betas[1],
                                             eps, weight_decay, _p(step), int(advance_step), _stream()), 'sn_fix_pair_adam')


def _lr_args(lr):
    """(float, device pointer or None): a one-element fp32 device tensor is handed over as lr_dev (read when the kernel
    runs, so captured launches follow a scheduler), a Python number as the immediate."""
    if isinstance(lr, Tensor):
        assert lr.dtype == torch.float32 and lr.numel() == 1 and lr.is_cuda
        return 0.0, _f32(lr)
    return float(lr), None


def adam(p: Tensor, g: Tensor, m: Tensor, v: Tensor, step: Tensor, lr, betas=(0.9, 0.999),
         eps: float = 1e-8, weight_decay: float = 0.0):
    """`step`: int64[2] on the device -- [0] the step counter (incremented by the launch), [1] a ticket word (0 between calls).
    `lr`: a Python number, or a one-element fp32 device tensor read at execution time (mcgen_adam's lr_dev)."""
    assert step.dtype == torch.int64 and step.numel() == 2
    lr_f, lr_dev = _lr_args(lr)
    check(_lib.load().mcgen_adam(_f32(p), _f32(g), _f32(m), _f32(v), p.numel(), lr_f, lr_dev, betas[0], betas[1], eps,
                                 weight_decay, _p(step), _stream()), 'adam')


def sgd(p: Tensor, g: Tensor, buf: Optional[Tensor], step: Tensor, lr, momentum: float = 0.0, weight_decay: float = 0.0):
    """mcgen_sgd: torch.optim.SGD (no dampening, no Nesterov).  `buf`: the momentum buffer, None when momentum == 0.
    `step` and `lr` as in ops.adam."""
    assert step.dtype == torch.int64 and step.numel() == 2
    lr_f, lr_dev = _lr_args(lr)
    check(_lib.load().mcgen_sgd(_f32(p), _f32(g), _f32(buf), p.numel(), lr_f, lr_dev, momentum,
                                weight_decay, _p(step), _stream()), 'sgd')


def rmsprop(p: Tensor, g: Tensor, square_avg: Tensor, buf: Optional[Tensor], step: Tensor, lr, alpha: float = 0.99,
            eps: float = 1e-8, momentum: float = 0.0, weight_decay: float = 0.0):
    """mcgen_rmsprop: torch.optim.RMSprop (not centered).  `buf`: the momentum buffer, None when momentum == 0.
    `step` and `lr` as in ops.adam."""
    assert step.dtype == torch.int64 and step.numel() == 2
    lr_f, lr_dev = _lr_args(lr)
    check(_lib.load().mcgen_rmsprop(_f32(p), _f32(g), _f32(square_avg), _f32(buf), p.numel(), lr_f,
                                    lr_dev, alpha, eps, momentum, weight_decay, _p(step), _stream()), 'rmsprop')


def adamax(p: Tensor, g: Tensor, m: Tensor, u: Tensor, step: Tensor, lr, betas=(0.9, 0.999), eps: float = 1e-8,
           weight_decay: float = 0.0):
    """mcgen_adamax: torch.optim.Adamax (`m`: exp_avg, `u`: exp_inf).  `step` and `lr` as in ops.adam."""
    assert step.dtype == torch.int64 and step.numel() == 2
    lr_f, lr_dev = _lr_args(lr)
    check(_lib.load().mcgen_adamax(_f32(p), _f32(g), _f32(m), _f32(u), p.numel(), lr_f, lr_dev, betas[0], betas[1], eps,
                                   weight_decay, _p(step), _stream()), 'adamax')


def ema_update(ema: Tensor, p: Tensor, step: Tensor, decay: float, start: int = 0, advance: bool = True):
    """mcgen_ema_update over two flat fp32 ranges of one length: ema = p (bit for bit) while step[0] < start, else
    ema = decay * ema + (1 - decay) * p.  `step`: int64[2] {counter, ticket} as in ops.adam, read when the kernel runs;
    `advance`: this launch increments the counter (the last launch of an update that takes several)."""
    assert step.dtype == torch.int64 and step.numel() == 2
    assert ema.numel() == p.numel()
    check(_lib.load().mcgen_ema_update(_f32(ema), _f32(p), p.numel(), decay, int(start), _p(step), int(advance),
                                       _stream()), 'ema_update')


def swap_(a: Tensor, b: Tensor):
    """mcgen_swap_f32: exchange two flat fp32 ranges of one length in place, bit for bit (no third buffer, no pointer moves)."""
    assert a.numel() == b.numel()
    check(_lib.load().mcgen_swap_f32(_f32(a), _f32(b), a.numel(), _stream()), 'swap_f32')


# ---- batched small launches (one launch per network pass instead of one per layer) ----------------------
def _struct_table(arr, device) -> Tensor:
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


class PrepJob(NamedTuple):
    """One weight-image job: master weight `w` -> the persistent buffer `image`."""
    w: Tensor
    image: Tensor
    transpose: bool = False
    row_perm: int = 1
    sigma_idx: int = -1                  # index into the sigma vector of PrepBatch.run, or -1
    wscale: float = 1.0
    kmajor: bool = False                 # K-major image (mode-compacted launches)
    kmap: Optional[Tensor] = None        # a mode's compacted image: input channel k <- kmap[k], k < kcount
    kcount: int = 0
    rmap: Optional[Tensor] = None        # image row r <- weight row rmap[r] (mcgen_conv_t.yperm)


class PrepBatch:
    """A fixed list of weight-image jobs run as ONE launch.  A job is a PrepJob; a plain tuple in PrepJob's field order
    (trailing fields left out take their defaults) is read as one."""

    def __init__(self, jobs: Sequence[PrepJob], dtype: torch.dtype):
        self.dtype = dtype
        jobs = [PrepJob(*j) for j in jobs]
        self.jobs = jobs = [j._replace(w=j.w.detach(), kcount=int(j.kcount) if j.kmap is not None else 0) for j in jobs]
        arr = (_lib.Prep * len(jobs))()
        for d, (w, img, transpose, row_perm, sidx, wscale, kmajor, kmap, kcount, rmap) in zip(arr, jobs):
            cout, cin = w.shape[0], w.shape[1]
            ks = w.shape[2] if w.dim() == 4 else 1
            if kmap is not None:
                assert not kmajor and not transpose and row_perm == 1 and kmap.dtype == torch.int16 and kmap.numel() >= kcount
                want = weight_image_elems(cout, kcount, ks, False)
            else:
                want = weight_image_k_elems(cout, cin, ks) if kmajor else weight_image_elems(cout, cin, ks, transpose)
            assert img.numel() == want and img.dtype == dtype and not (kmajor and (transpose or row_perm != 1))
            d.w, d.image = _f32(w), _p(img)
            d.Cout, d.Cin, d.ksize, d.transpose, d.row_perm, d.sigma_idx = cout, cin, ks, int(transpose), row_perm, sidx
            d.wscale, d.layout = float(wscale), int(kmajor)
            d.kmap, d.kcount = _p(kmap), kcount
            if rmap is not None:
                assert not kmajor and not transpose and row_perm == 1 and rmap.dtype == torch.int16 and rmap.numel() >= cout and rmap.is_contiguous()
            d.rmap = _p(rmap)
        self.key = tuple((w.data_ptr(), img.data_ptr()) for w, img, *_ in jobs)
        self.table = _struct_table(arr, jobs[0].w.device)
        self.n = len(jobs)

    def valid(self) -> bool:
        return self.key == tuple((w.data_ptr(), img.data_ptr()) for w, img, *_ in self.jobs)

    def run(self, sigma: Optional[Tensor] = None):
        check(_lib.load().mcgen_prep_weight_batch(_p(self.table), self.n, _f32(sigma), _dt(self.dtype), _stream()),
              'prep_weight_batch')


def prep_and_codes(prep: 'PrepBatch', sigma: Optional[Tensor], codes: 'CodeBatch', label: Tensor, reps: int = 1,
                   scale: Optional[Tensor] = None, n_half: int = 0):
    """PrepBatch.run(sigma) and CodeBatch.run_labels(label, reps, scale, n_half) as ONE launch (mcgen_prep_weight_batch_codes):
    a discriminator pass's weight images and codes both wait for the power iteration only.  -> the code tensors."""
    codes._ensure()
    n = label.shape[0] * reps
    codes._tables_for(n, label.device)
    if label.dtype != torch.int64 or any(d.C % 4 for d in codes._arr):
        raise _lib.McgenError('prep_and_codes: int64 labels and channel counts that are multiples of 4')
    buf = torch.empty(codes._total, dtype=torch.float32, device=label.device)
    check(_lib.load().mcgen_prep_weight_batch_codes(_p(prep.table), prep.n, _f32(sigma), _dt(prep.dtype), _p(label.contiguous()),
                                                    label.shape[0], _p(codes._table), len(codes.mcs), _f32(buf), n, _f32(scale), n_half,
                                                    _stream()), 'prep_weight_batch_codes')
    out, off = [], 0
    for d in codes._arr:
        out.append(buf[off:off + n * d.C].view(n, d.C))
        off += n * d.C
    return out


class CodeBatch:
    """Codes of a list of MultimodalController modules in ONE launch; rebuilt when a codebook buffer was
    re-registered (models.utils.create / transit) or moved."""

    def __init__(self, mcs, scale_idx=None):
        """`mcs`: modules with a `codebook` buffer; `scale_idx[i]` (optional): index into the `scale` vector given to
        run() whose entry multiplies the rows n >= n_half of job i (-1: none)."""
        self.mcs = list(mcs)
        self.scale_idx = list(scale_idx) if scale_idx is not None else [-1] * len(self.mcs)
        self._key = None

    def _ensure(self):
        key = tuple((m.codebook.data_ptr(), tuple(m.codebook.shape)) for m in self.mcs)
        if key != self._key:
            arr = (_lib.Code * len(self.mcs))()
            off = 0
            self.offsets = []
            for d, m in zip(arr, self.mcs):
                cb = m.codebook
                if cb.dtype != torch.float32 or not cb.is_contiguous():
                    raise _lib.McgenError('codebook must be a contiguous float32 buffer')
                d.codebook, d.out_off, d.M, d.C = _p(cb), off, cb.shape[0], cb.shape[1]
                d.scale_idx = self.scale_idx[len(self.offsets)]
                self.offsets.append((off, cb.shape[1]))
                off += 0                                   # per-forward: offsets scale with N, filled in run()
            self._arr = arr
            self._key = key
            self._n_cached = None

    def run_labels(self, label: Tensor, reps: int = 1, scale: Optional[Tensor] = None, n_half: int = 0):
        """The same for one-hot indicators given as int64 labels: code_i = codebook_i[label] (a row gather per module, all in
        one launch: mcgen_mc_gather_batch).  `reps`: the batch is the label vector `reps` times back to back; `scale` /
        `n_half` as in run()."""
        self._ensure()
        n = label.shape[0] * reps
        self._tables_for(n, label.device)
        if label.dtype != torch.int64 or any(d.C % 4 for d in self._arr):
            raise _lib.McgenError('run_labels: int64 labels and channel counts that are multiples of 4')
        buf = torch.empty(self._total, dtype=torch.float32, device=label.device)
        check(_lib.load().mcgen_mc_gather_batch(_p(label.contiguous()), label.shape[0], _p(self._table), len(self.mcs), _f32(buf), n,
                                                _f32(scale), n_half, _stream()), 'mc_gather_batch')
        out, off = [], 0
        for d in self._arr:
            out.append(buf[off:off + n * d.C].view(n, d.C))
            off += n * d.C
        return out

    def _hinted(self, indicator: Tensor):
        """(label, reps) when `indicator` carries its labels (`onehot_hint`) and run_labels takes them -- int64 device labels
        that cover the batch, channel counts that are multiples of 4 -- else None."""
        hint = getattr(indicator, '_mcgen_onehot', None)
        if hint is not None and hint[0].shape[0] * hint[1] == indicator.shape[0] and hint[0].is_cuda and hint[0].dtype == torch.int64 \
                and all(d.C % 4 == 0 for d in (self._ensure() or self._arr)):
            return hint[0], hint[1]
        return None

    def labels_of(self, indicator: Tensor):
        """(label, reps) when `indicator` carries its labels (`onehot_hint`) and run_labels applies, else None."""
        return self._hinted(indicator)

    def run_any(self, indicator: Tensor, scale: Optional[Tensor] = None, n_half: int = 0):
        """run(), or run_labels() when the indicator carries its labels (`onehot_hint`): the caller built it with
        F.one_hot / ops.onehot_rep, so a row gather gives indicator @ codebook exactly."""
        lab = self._hinted(indicator)
        if lab is not None:
            return self.run_labels(lab[0], lab[1], scale, n_half)
        return self.run(indicator, scale, n_half)

    def _tables_for(self, n: int, device):
        if self._n_cached != n:
            # one descriptor table per batch size (the paired discriminator pass alternates 2N and N)
            if not isinstance(getattr(self, '_tables', None), dict) or self._tables.get('key') != self._key:
                self._tables = {'key': self._key}
            if n not in self._tables:
                off = 0
                for d in self._arr:
                    d.out_off = off
                    off += n * d.C
                self._tables[n] = (off, _struct_table(self._arr, device))
            self._total, self._table = self._tables[n]
            self._n_cached = n

    def run(self, indicator: Tensor, scale: Optional[Tensor] = None, n_half: int = 0):
        """-> list of [N, C] code tensors (views of one buffer), in module order."""
        self._ensure()
        n = indicator.shape[0]
        self._tables_for(n, indicator.device)
        if indicator.shape[1] != self._arr[0].M:
            raise _lib.McgenError(f'indicator has {indicator.shape[1]} modes, codebook has {self._arr[0].M}')
        buf = torch.empty(self._total, dtype=torch.float32, device=indicator.device)
        check(_lib.load().mcgen_mc_code_batch(_f32(indicator.contiguous()), _p(self._table), len(self.mcs), _f32(buf), n,
                                              _f32(scale), n_half, _stream()), 'mc_code_batch')
        out, off = [], 0
        for d in self._arr:
            out.append(buf[off:off + n * d.C].view(n, d.C))
            off += n * d.C
        return out


# ---- MCGlow kernels ---------------------------------------------------------------------------------------------
def glow_squeeze(x: Tensor, c: int) -> Tensor:
    """[N,H,W,Cp] (c logical channels) -> [N,H/2,W/2,pad8(4c)]  (mcglow.py:221-223)."""
    n, h, w, cp = x.shape
    y = torch.empty((n, h // 2, w // 2, pad8(4 * c)), dtype=x.dtype, device=x.device)
    check(_lib.load().mcgen_glow_squeeze(_p(x), _p(y), _dt(x.dtype), n, h, w, c, cp, y.shape[-1], 0, _stream()), 'glow_squeeze')
    return y


def glow_unsqueeze(x: Tensor, c4: int) -> Tensor:
    """[N,H,W,Cp] with c4 = 4c logical channels -> [N,2H,2W,pad8(c)]  (mcglow.py:262-265)."""
    n, h, w, cp = x.shape
    c = c4 // 4
    y = torch.empty((n, 2 * h, 2 * w, pad8(c)), dtype=x.dtype, device=x.device)
    check(_lib.load().mcgen_glow_squeeze(_p(x), _p(y), _dt(x.dtype), n, 2 * h, 2 * w, c, y.shape[-1], cp, 1, _stream()), 'glow_unsqueeze')
    return y


def channel_stats(x: Tensor, blocks: int = 64) -> Tensor:
    cp = x.shape[-1]
    pixels = x.numel() // cp
    blocks = max(1, min(blocks, pixels))
    part = torch.empty((blocks, 2, cp), dtype=torch.float32, device=x.device)
    check(_lib.load().mcgen_channel_stats(_p(x), _dt(x.dtype), pixels, cp, _f32(part), blocks, _stream()), 'channel_stats')
    return part


def actnorm_init(partials: Tensor, count: int, loc: Tensor, scale: Tensor):
    """ActNorm.initialize (mcglow.py:32-39) into the parameter tensors loc / scale ([1,C,1,1])."""
    tiles, _, pitch = partials.shape
    check(_lib.load().mcgen_actnorm_init(_f32(partials), tiles, pitch, loc.numel(), float(count), _f32(loc), _f32(scale),
                                         _stream()), 'actnorm_init')


def actnorm_affine(loc: Tensor, scale: Tensor, cp: int, with_negloc: bool = False):
    """Prologue vectors of the op that consumes an ActNorm: y = x * a + b with a = scale, b = scale * loc (zero-padded to
    cp); with_negloc also returns -loc (the gate mean of the backward pass)."""
    c = loc.numel()
    ab = torch.empty((3 if with_negloc else 2, cp), dtype=torch.float32, device=loc.device)
    check(_lib.load().mcgen_actnorm_affine(_f32(loc), _f32(scale), c, cp, ab[0].data_ptr(), ab[1].data_ptr(),
                                           ab[2].data_ptr() if with_negloc else None, _stream()), 'actnorm_affine')
    return (ab[0], ab[1], ab[2]) if with_negloc else (ab[0], ab[1])


def glow_param_logdet(scale: Tensor, w_s: Tensor, hw: int, logdet: Tensor):
    check(_lib.load().mcgen_glow_param_logdet(_f32(scale), scale.numel(), _f32(w_s), w_s.numel(), float(hw), _f32(logdet),
                                              logdet.numel(), _stream()), 'glow_param_logdet')


def invconv_weight(w_p, w_l, w_u, w_s, s_sign, inverse: bool = False):
    c = w_s.numel()
    w = torch.empty((c, c), dtype=torch.float32, device=w_s.device)
    winv = torch.empty_like(w) if inverse else None
    check(_lib.load().mcgen_invconv_weight(_f32(w_p), _f32(w_l), _f32(w_u), _f32(w_s), _f32(s_sign), c, _f32(w), _f32(winv),
                                           _stream()), 'invconv_weight')
    return w, winv


# ---- batched MCGlow per-module ops (one launch per kind for all modules of a pass) --------------------------------------
def actnorm_affine_batch(ans, cps):
    """[(a, b, negloc)] for ActNorm modules `ans` (loc / scale parameters) padded to `cps[i]` channels: ONE buffer, one launch
    per MCGEN_GLOW_BATCH_MAX modules (mcgen_actnorm_affine_batch)."""
    dev = ans[0].loc.device
    buf = torch.empty(3 * sum(cps), dtype=torch.float32, device=dev)
    arr = (_lib.AnAffine * len(ans))()
    out, off = [], 0
    for d, an, cp in zip(arr, ans, cps):
        a, b, nl = buf[off:off + cp], buf[off + cp:off + 2 * cp], buf[off + 2 * cp:off + 3 * cp]
        off += 3 * cp
        d.loc, d.scale, d.a, d.b, d.negloc, d.C, d.Cp = _f32(an.loc.data), _f32(an.scale.data), _f32(a), _f32(b), _f32(nl), an.loc.numel(), cp
        out.append((a, b, nl))
    check(_lib.load().mcgen_actnorm_affine_batch(arr, len(ans), _stream()), 'actnorm_affine_batch')
    return out


def glow_param_logdet_batch(items, logdet: Tensor):
    """logdet[n] += sum over `items` = [(actnorm scale, w_s, H * W)] of HW * (sum log|scale| + sum w_s), one launch."""
    arr = (_lib.Pld * len(items))()
    for d, (scale, w_s, hw) in zip(arr, items):
        d.scale, d.w_s, d.C, d.Cw, d.hw = _f32(scale), _f32(w_s), scale.numel(), w_s.numel(), float(hw)
    check(_lib.load().mcgen_glow_param_logdet_batch(arr, len(items), _f32(logdet), logdet.numel(), _stream()), 'glow_param_logdet_batch')


def invconv_weight_batch(ics):
    """[W] of InvConv2dLU modules `ics` (mcglow.py:105-111), one launch per MCGEN_GLOW_BATCH_MAX modules."""
    arr = (_lib.Icw * len(ics))()
    out = []
    for d, ic in zip(arr, ics):
        c = ic.w_s.numel()
        w = torch.empty((c, c), dtype=torch.float32, device=ic.w_s.device)
        d.w_p, d.w_l, d.w_u, d.w_s, d.s_sign, d.weight, d.weight_inv, d.C = (_f32(ic.w_p), _f32(ic.w_l.data), _f32(ic.w_u.data),
                                                                            _f32(ic.w_s.data), _f32(ic.s_sign), _f32(w), None, c)
        out.append(w)
    check(_lib.load().mcgen_invconv_weight_batch(arr, len(ics), _stream()), 'invconv_weight_batch')
    return out


class GlowDeferred:
    """Parameter-gradient reductions of an MCGlow backward pass that nothing later in the pass reads (ActNorm loc / scale from
    the dgrad epilogues' partial sums, ZeroConv2d scale, the LU parameters): queued while the pass runs, launched batched at
    its end -- they were ~250 launches of 3-6 us."""

    def __init__(self):
        self.an, self.pcs, self.icb, self.icp, self.keep = [], [], [], [], []

    def actnorm_bwd(self, partials, scale, ld_coef, input_side, dloc, dscale, accumulate=False):
        self.an.append((partials, scale, float(ld_coef), int(input_side), dloc, dscale, int(accumulate)))

    def prod_colsum(self, a, b, c, out, alpha=1.0, accumulate=False):
        self.pcs.append((a, b, c, out, float(alpha), int(accumulate)))

    def invconv_bwd(self, ic, dW, ld_coef, dw_l, dw_u, dw_s, accumulate=False):
        self.icb.append((ic, dW, float(ld_coef), dw_l, dw_u, dw_s, int(accumulate)))

    def invconv_plain_bwd(self, dW, weight_inv, ld_coef, grad, accumulate=False):
        self.icp.append((dW, weight_inv, float(ld_coef), grad, int(accumulate)))

    def run(self):
        lib = _lib.load()
        if self.an:
            arr = (_lib.AnBwd * len(self.an))()
            for d, (p, sc, ld, side, dl, ds, acc) in zip(arr, self.an):
                tiles, _, pitch = p.shape
                d.partials, d.scale, d.dloc, d.dscale = _f32(p), _f32(sc), _f32(dl), _f32(ds)
                d.tiles, d.pitch, d.C, d.input_side, d.accumulate, d.ld_coef = tiles, pitch, sc.numel(), side, acc, ld
            check(lib.mcgen_actnorm_bwd_batch(arr, len(self.an), _stream()), 'actnorm_bwd_batch')
        if self.pcs:
            dt = self.pcs[0][0].dtype
            arr = (_lib.Pcs * len(self.pcs))()
            cmax = max(j[2] for j in self.pcs)
            for d, (a, b, c, out, alpha, acc) in zip(arr, self.pcs):
                assert a.dtype == dt and b.dtype == dt
                d.a, d.b, d.out, d.pixels = _p(a), _p(b), _f32(out), a.numel() // a.shape[-1]
                d.pitch_a, d.pitch_b, d.C, d.accumulate, d.alpha = a.shape[-1], b.shape[-1], c, acc, alpha
            ws = torch.empty(len(self.pcs) * 256 * cmax, dtype=torch.float32, device=self.pcs[0][0].device)
            check(lib.mcgen_prod_colsum_batch(arr, len(self.pcs), _dt(dt), _f32(ws), _stream()), 'prod_colsum_batch')
        if self.icb:
            arr = (_lib.Icb * len(self.icb))()
            for d, (ic, dW, ld, dl, du, dsg, acc) in zip(arr, self.icb):
                d.w_p, d.w_l, d.w_u, d.w_s, d.s_sign = _f32(ic.w_p), _f32(ic.w_l.data), _f32(ic.w_u.data), _f32(ic.w_s.data), _f32(ic.s_sign)
                d.dW, d.dw_l, d.dw_u, d.dw_s = _f32(dW), _f32(dl), _f32(du), _f32(dsg)
                d.C, d.ldw, d.accumulate, d.ld_coef = ic.w_s.numel(), dW.shape[-1], acc, ld
            check(lib.mcgen_invconv_bwd_batch(arr, len(self.icb), _stream()), 'invconv_bwd_batch')
        if self.icp:
            invconv_plain_bwd_batch(self.icp)
        self.an, self.pcs, self.icb, self.icp = [], [], [], []


def prep_weight_rows(w: Tensor, dtype: torch.dtype, row_scale: Tensor) -> Tensor:
    cout, cin = w.shape[0], w.shape[1]
    ks = w.shape[2] if w.dim() == 4 else 1
    out = torch.empty(weight_image_elems(cout, cin, ks, False), dtype=dtype, device=w.device)
    check(_lib.load().mcgen_prep_weight_rows(_f32(w.contiguous()), _p(out), _dt(dtype), cout, cin, ks, _f32(row_scale), _stream()),
          'prep_weight_rows')
    return out


def glow_coupling(x: Tensor, h: Tensor, c: int, logdet: Optional[Tensor], reverse: bool = False, accumulate: bool = True) -> Tensor:
    n, cp = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * cp)
    assert h.shape == x.shape and h.dtype == x.dtype
    y = torch.empty_like(x)
    check(_lib.load().mcgen_glow_coupling(_p(x), _p(h), _p(y), _dt(x.dtype), _f32(logdet), n, hw, c, cp, int(reverse),
                                          int(accumulate), _stream()), 'glow_coupling')
    return y


def gaussian_logp(z: Tensor, c0: int, prior: Tensor, cz: int, logp: Tensor, accumulate: bool = True):
    n = z.shape[0]
    hw = z.numel() // (n * z.shape[-1])
    check(_lib.load().mcgen_gaussian_logp(_p(z), z.shape[-1], c0, _p(prior), prior.shape[-1], _dt(z.dtype), n, hw, cz,
                                          _f32(logp), int(accumulate), _stream()), 'gaussian_logp')


def gaussian_sample(eps: Tensor, prior: Tensor, out: Tensor, c0: int, cz: int):
    pixels = eps.numel() // eps.shape[-1]
    check(_lib.load().mcgen_gaussian_sample(_p(eps), eps.shape[-1], _p(prior), prior.shape[-1], _p(out), out.shape[-1], c0,
                                            _dt(eps.dtype), pixels, cz, _stream()), 'gaussian_sample')


def copy_channels(src: Tensor, s0: int, dst: Tensor, c0: int, cn: int):
    pixels = src.numel() // src.shape[-1]
    check(_lib.load().mcgen_copy_channels(_p(src), src.shape[-1], s0, _p(dst), dst.shape[-1], c0, _dt(src.dtype), pixels, cn,
                                          _stream()), 'copy_channels')


def glow_coupling_bwd(v: Tensor, h: Tensor, dy: Tensor, c: int, g: float):
    dv, dh = torch.empty_like(v), torch.empty_like(v)
    pixels = v.numel() // v.shape[-1]
    check(_lib.load().mcgen_glow_coupling_bwd(_p(v), _p(h), _p(dy), _p(dv), _p(dh), _dt(v.dtype), float(g), pixels, c,
                                              v.shape[-1], _stream()), 'glow_coupling_bwd')
    return dv, dh


def gaussian_logp_bwd(z: Tensor, c0: int, prior: Tensor, cz: int, dz: Tensor, d0: int, g: float, accumulate_dz: bool):
    dprior = torch.zeros_like(prior)
    pixels = z.numel() // z.shape[-1]
    check(_lib.load().mcgen_gaussian_logp_bwd(_p(z), z.shape[-1], c0, _p(prior), prior.shape[-1], _p(dz), dz.shape[-1], d0,
                                              _p(dprior), _dt(z.dtype), float(g), pixels, cz, int(accumulate_dz), _stream()),
          'gaussian_logp_bwd')
    return dprior


def prod_colsum(a: Tensor, b: Tensor, c: int, out: Tensor, alpha: float = 1.0, accumulate: bool = False):
    pixels = a.numel() // a.shape[-1]
    ws = torch.empty(256 * c, dtype=torch.float32, device=a.device)
    check(_lib.load().mcgen_prod_colsum(_p(a), a.shape[-1], _p(b), b.shape[-1], _dt(a.dtype), pixels, c, _f32(out), float(alpha),
                                        int(accumulate), _f32(ws), _stream()), 'prod_colsum')


def actnorm_bwd(partials: Tensor, scale: Tensor, ld_coef: float, input_side: bool, dloc: Tensor, dscale: Tensor,
                accumulate: bool = False):
    tiles, _, pitch = partials.shape
    check(_lib.load().mcgen_actnorm_bwd(_f32(partials), tiles, pitch, scale.numel(), _f32(scale), float(ld_coef),
                                        int(input_side), _f32(dloc), _f32(dscale), int(accumulate), _stream()), 'actnorm_bwd')


def invconv_bwd(w_p, w_l, w_u, w_s, s_sign, dW: Tensor, ld_coef: float, dw_l, dw_u, dw_s, accumulate: bool = False):
    c = w_s.numel()
    check(_lib.load().mcgen_invconv_bwd(_f32(w_p), _f32(w_l), _f32(w_u), _f32(w_s), _f32(s_sign), _f32(dW), c, dW.shape[-1],
                                        float(ld_coef), _f32(dw_l), _f32(dw_u), _f32(dw_s), int(accumulate), _stream()),
          'invconv_bwd')


# ---- the other two forms of a flow: plain InvConv2d (glow.conv_lu = False), additive coupling (glow.affine = False) ---------
def _square_weight(weight: Tensor, what: str) -> int:
    """C of an InvConv2d weight [C, C] or [C, C, 1, 1] (read densely); refuses what the kernel cannot take."""
    if weight.dim() not in (2, 4) or weight.shape[0] != weight.shape[1] or weight.numel() != weight.shape[0] ** 2:
        raise _lib.McgenError(f'{what}: expected a [C, C] or [C, C, 1, 1] weight, got {tuple(weight.shape)}')
    c = weight.shape[0]
    if not 1 <= c <= 64:
        raise _lib.McgenError(f'{what}: C must be in 1..64, got {c}')
    return c


def invconv_plain(weight: Tensor):
    """(logabsdet [1], weight_inv [C, C]) of an InvConv2d weight (mcglow.py:69,73), factorised in float64."""
    c = _square_weight(weight, 'invconv_plain')
    lad = torch.empty(1, dtype=torch.float32, device=weight.device)
    winv = torch.empty((c, c), dtype=torch.float32, device=weight.device)
    check(_lib.load().mcgen_invconv_plain(_f32(weight), c, _f32(lad), _f32(winv), _stream()), 'invconv_plain')
    return lad, winv


def invconv_plain_batch(weights):
    """[(logabsdet [1], weight_inv [C, C])] of InvConv2d weights, one launch per MCGEN_GLOW_BATCH_MAX matrices: the
    log-determinants share one buffer, the inverses another."""
    cs = [_square_weight(w, 'invconv_plain_batch') for w in weights]
    dev = weights[0].device
    lads = torch.empty(len(cs), dtype=torch.float32, device=dev)
    invs = torch.empty(sum(c * c for c in cs), dtype=torch.float32, device=dev)
    arr = (_lib.Icp * len(cs))()
    out, off = [], 0
    for i, (d, w, c) in enumerate(zip(arr, weights, cs)):
        lad, winv = lads[i:i + 1], invs[off:off + c * c].view(c, c)
        off += c * c
        d.weight, d.logabsdet, d.weight_inv, d.C = _f32(w), _f32(lad), _f32(winv), c
        out.append((lad, winv))
    check(_lib.load().mcgen_invconv_plain_batch(arr, len(cs), _stream()), 'invconv_plain_batch')
    return out


def _plain_bwd_args(dW: Tensor, weight_inv: Tensor, grad: Tensor, what: str):
    c = _square_weight(weight_inv, what)
    if dW.dim() != 2 or dW.shape[0] != c or dW.shape[1] < c:
        raise _lib.McgenError(f'{what}: dW must be [C, ldw >= C] with C = {c}, got {tuple(dW.shape)}')
    if grad.numel() != c * c:
        raise _lib.McgenError(f'{what}: grad must hold C * C = {c * c} elements, got {tuple(grad.shape)}')
    return c, dW.shape[1]


def invconv_plain_bwd(dW: Tensor, weight_inv: Tensor, ld_coef: float, grad: Tensor, accumulate: bool = False):
    """grad (+)= dW[:, :C] + ld_coef * weight_inv^T: the InvConv2d weight gradient from the reduced 1x1 weight gradient dW
    [C, ldw] and d log|det W| / dW = W^-T."""
    c, ldw = _plain_bwd_args(dW, weight_inv, grad, 'invconv_plain_bwd')
    check(_lib.load().mcgen_invconv_plain_bwd(_f32(dW), c, ldw, _f32(weight_inv), float(ld_coef), _f32(grad), int(accumulate),
                                              _stream()), 'invconv_plain_bwd')


def invconv_plain_bwd_batch(jobs):
    """`jobs`: [(dW, weight_inv, ld_coef, grad, accumulate)], one launch per MCGEN_GLOW_BATCH_MAX jobs."""
    arr = (_lib.Icpb * len(jobs))()
    for d, (dW, winv, ld, grad, acc) in zip(arr, jobs):
        c, ldw = _plain_bwd_args(dW, winv, grad, 'invconv_plain_bwd_batch')
        d.dW, d.weight_inv, d.grad, d.C, d.ldw, d.accumulate, d.ld_coef = _f32(dW), _f32(winv), _f32(grad), c, ldw, int(acc), float(ld)
    check(_lib.load().mcgen_invconv_plain_bwd_batch(arr, len(jobs), _stream()), 'invconv_plain_bwd_batch')


def glow_coupling_add(x: Tensor, h: Tensor, c: int, reverse: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """Additive coupling (mcglow.py:160-163 / 172-174): y = [x_a | x_b +- h] on [N, H, W, Cp] with h the coupling network's
    C/2 channels (its own pitch); channels >= C of y are zero.  `out` may be x itself."""
    cp, ch = x.shape[-1], h.shape[-1]
    y = torch.empty_like(x) if out is None else out
    if c <= 0 or c % 2 or cp < c or cp % 8 or ch < c // 2:
        raise _lib.McgenError(f'glow_coupling_add: C = {c} must be even, Cp = {cp} a multiple of 8 >= C, Ch = {ch} >= C / 2')
    if h.dtype != x.dtype or y.dtype != x.dtype or h.shape[:-1] != x.shape[:-1] or y.shape != x.shape:
        raise _lib.McgenError('glow_coupling_add: x, h and y must share dtype and pixels')
    check(_lib.load().mcgen_glow_coupling_add(_p(x), _p(h), _p(y), _dt(x.dtype), x.numel() // cp, c, cp, ch, -1 if reverse else 1,
                                              _stream()), 'glow_coupling_add')
    return y


def clip_grad_norm_(gflat: Tensor, max_norm: float) -> Tensor:
    """torch.nn.utils.clip_grad_norm_ over one flat gradient buffer; returns the total norm (device scalar)."""
    ws = torch.empty(256 + 1, dtype=torch.float32, device=gflat.device)
    check(_lib.load().mcgen_clip_grad_norm(_f32(gflat), gflat.numel(), float(max_norm), ws[256:].data_ptr(), _f32(ws),
                                           _stream()), 'clip_grad_norm')
    return ws[256]


# --------------------------------------------------------------------------- #
# MCPixelCNN (models/mcpixelcnn.py)
def im2col(x: Tensor, kh: int, kw: int, oh: int, ow: int, stride: int = 1, scale: Optional[Tensor] = None,
           shift: Optional[Tensor] = None, relu: bool = False, code: Optional[Tensor] = None) -> Tensor:
    """[N,H,W,Cp] -> [N,H/stride,W/stride,kh*kw*Cp] of the (optionally activated) input; see mcgen_im2col."""
    n, h, w, cp = x.shape
    col = torch.empty((n, h // stride, w // stride, kh * kw * cp), dtype=x.dtype, device=x.device)
    if code is not None and tuple(code.shape) != (n, cp):
        raise _lib.McgenError(f'im2col: code must be {(n, cp)}')
    check(_lib.load().mcgen_im2col(_p(x), _p(col), _dt(x.dtype), n, h, w, cp, kh, kw, oh, ow, stride, _f32(scale), _f32(shift),
                                   int(relu), _f32(code), _stream()), 'im2col')
    return col


def col2im(dcol: Tensor, cp: int, kh: int, kw: int, oh: int, ow: int, stride: int = 1, bias: Optional[Tensor] = None,
           out: Optional[Tensor] = None) -> Tensor:
    """Adjoint of im2col: [N,Ho,Wo,kh*kw*cp] -> [N,Ho*stride,Wo*stride,cp] (+ bias); accumulates into `out` if given."""
    n, ho, wo, _ = dcol.shape
    acc = out is not None
    if out is None:
        out = torch.empty((n, ho * stride, wo * stride, cp), dtype=dcol.dtype, device=dcol.device)
    check(_lib.load().mcgen_col2im(_p(dcol), _p(out), _dt(dcol.dtype), n, ho * stride, wo * stride, cp, kh, kw, oh, ow, stride,
                                   _f32(bias), bias.numel() if bias is not None else 0, int(acc), _stream()), 'col2im')
    return out


def gated_fwd(s: Tensor, scale: Tensor, shift: Tensor, code: Tensor) -> Tensor:
    n, h, w, c2 = s.shape
    c = c2 // 2
    out = torch.empty((n, h, w, c), dtype=s.dtype, device=s.device)
    check(_lib.load().mcgen_gated_fwd(_p(s), _f32(scale), _f32(shift), _f32(code), _p(out), _dt(s.dtype), n, h * w, c, _stream()),
          'gated_fwd')
    return out


def gated_fwd_batch(items):
    """items = [(s, scale, shift, code)]: independent gated activations in ONE launch (mcgen_gated_fwd_batch, <= 4) -> [out]."""
    arr = (_lib.Gated * len(items))()
    outs = []
    for d, (s, scale, shift, code) in zip(arr, items):
        n, h, w, c2 = s.shape
        out = torch.empty((n, h, w, c2 // 2), dtype=s.dtype, device=s.device)
        d.s, d.scale, d.shift, d.code, d.out = _p(s), _f32(scale), _f32(shift), _f32(code), _p(out)
        d.N, d.HW, d.C = n, h * w, c2 // 2
        outs.append(out)
    check(_lib.load().mcgen_gated_fwd_batch(arr, len(items), _dt(items[0][0].dtype), _stream()), 'gated_fwd_batch')
    return outs


def _bwd_sums(partials: Tensor, c: int, dgamma: Optional[Tensor], dbeta: Optional[Tensor]) -> Tensor:
    tiles, _, pitch = partials.shape
    sums = torch.empty((2, c), dtype=torch.float32, device=partials.device)
    check(_lib.load().mcgen_bn_bwd_finalize(_f32(partials), tiles, pitch, c, _f32(dgamma), _f32(dbeta), _f32(sums), 0, _stream()),
          'bn_bwd_finalize')
    return sums


def gated_bwd(s: Tensor, scale, shift, mean, rstd, code: Tensor, g: Tensor, dgamma: Tensor, dbeta: Tensor) -> Tensor:
    """Backward of gated_fwd through the batch statistics: returns ds [.., 2C]; fills dgamma / dbeta."""
    n, h, w, c2 = s.shape
    c = c2 // 2
    pixels = n * h * w
    blocks = max(1, min(256, pixels // 16))
    ds = torch.empty_like(s)
    part = torch.empty((blocks, 2, c), dtype=torch.float32, device=s.device)
    lib = _lib.load()
    check(lib.mcgen_gated_bwd_stats(_p(s), _f32(scale), _f32(shift), _f32(mean), _f32(rstd), _f32(code), _p(g), _p(ds), _f32(part),
                                    blocks, _dt(s.dtype), n, h * w, c, _stream()), 'gated_bwd_stats')
    sums = _bwd_sums(part, c, dgamma, dbeta)
    check(lib.mcgen_gated_bwd_apply(_p(ds), _p(s), _f32(sums), _f32(scale), _f32(mean), _f32(rstd), float(pixels), _dt(s.dtype),
                                    pixels, c, _stream()), 'gated_bwd_apply')
    return ds


def affine_code_res(x: Tensor, scale, shift, code: Optional[Tensor], res: Optional[Tensor], pre_relu: bool = False,
                    post_relu: bool = False) -> Tensor:
    """y = post_relu?( pre_relu?(x*scale + shift) * code + res ); x is [N, ..., C], code [N, C]."""
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    y = torch.empty_like(x)
    check(_lib.load().mcgen_affine_code_res(_p(x), _f32(scale), _f32(shift), _f32(code), _p(res), _p(y), _dt(x.dtype), n, hw, c,
                                            int(pre_relu), int(post_relu), _stream()), 'affine_code_res')
    return y


def affine_relu_maxpool2(x: Tensor, scale: Tensor, shift: Tensor) -> Tensor:
    """MaxPool2d(2)(relu(x * scale + shift)) on [N, H, W, C] (mcgen_affine_relu_maxpool2)."""
    n, h, w, c = x.shape
    if h % 2 or w % 2 or scale.numel() != c or shift.numel() != c:
        raise _lib.McgenError(f'affine_relu_maxpool2: even H, W and [C] affine vectors, got {tuple(x.shape)} / {scale.numel()}')
    y = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
    check(_lib.load().mcgen_affine_relu_maxpool2(_p(x), _f32(scale), _f32(shift), _p(y), _dt(x.dtype), n, h // 2, w // 2, c, _stream()),
          'affine_relu_maxpool2')
    return y


def code_bn_bwd(g: Tensor, code: Optional[Tensor], x: Tensor, scale, mean, rstd, dgamma: Tensor, dbeta: Tensor,
                shift=None, pre_relu: bool = False, y_post: Optional[Tensor] = None, want_gated: bool = False):
    """Backward of y = post_relu?( pre_relu?(BN(x)) * code + res ) w.r.t. x (training-mode BatchNorm); fills
    dgamma / dbeta.  Returns dx, or (dx, g * [y_post > 0]) when want_gated (the residual's gradient)."""
    n, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (n * c)
    pixels = n * hw
    blocks = max(1, min(256, pixels // 16))
    dz = torch.empty_like(x)
    gated = torch.empty_like(x) if (want_gated and y_post is not None) else None
    part = torch.empty((blocks, 2, c), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    check(lib.mcgen_code_bn_stats(_p(g), _f32(code), _p(x), _f32(mean), _f32(rstd), _p(dz), _f32(part), blocks, _dt(x.dtype),
                                  n, hw, c, _f32(scale), _f32(shift), int(pre_relu), _p(y_post), _p(gated), _stream()),
          'code_bn_stats')
    sums = _bwd_sums(part, c, dgamma, dbeta)
    dx = torch.empty_like(x)
    check(lib.mcgen_bn_bwd_apply(_p(dz), _p(x), None, _p(dx), _dt(x.dtype), pixels, c, _f32(sums), float(pixels), _f32(scale),
                                 _f32(mean), _f32(rstd), _stream()), 'bn_bwd_apply')
    if want_gated:
        return dx, (gated if gated is not None else g)
    return dx


def maxpool2_bn_bwd(gp: Tensor, x: Tensor, scale, shift, mean, rstd, dgamma: Tensor, dbeta: Tensor) -> Tensor:
    """Backward of y = MaxPool2d(2)(relu(x * scale + shift)) through training-mode BatchNorm (the classifier's block tail,
    forward mcgen_affine_relu_maxpool2 with the batch affine) w.r.t. x [N, 2Ho, 2Wo, C]; fills dgamma / dbeta.  The
    window argmax is recomputed from x (first strict maximum, ReLU gate), so no index tensor and no full-size dz."""
    n, h, w, c = x.shape
    ho, wo = h // 2, w // 2
    if h % 2 or w % 2 or tuple(gp.shape) != (n, ho, wo, c) or gp.dtype != x.dtype:
        raise _lib.McgenError(f'maxpool2_bn_bwd: gp must be {(n, ho, wo, c)} {x.dtype}, got {tuple(gp.shape)} {gp.dtype}')
    blocks = max(1, min(256, (n * ho * wo) // 16))
    part = torch.empty((blocks, 2, c), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    check(lib.mcgen_maxpool2_bn_bwd_stats(_p(gp), _p(x), _f32(scale), _f32(shift), _f32(mean), _f32(rstd), _f32(part), blocks,
                                          _dt(x.dtype), n, ho, wo, c, _stream()), 'maxpool2_bn_bwd_stats')
    sums = _bwd_sums(part, c, dgamma, dbeta)
    dx = torch.empty_like(x)
    check(lib.mcgen_maxpool2_bn_bwd_apply(_p(gp), _p(x), _f32(scale), _f32(shift), _f32(mean), _f32(rstd), _f32(sums), _p(dx),
                                          _dt(x.dtype), n, ho, wo, c, _stream()), 'maxpool2_bn_bwd_apply')
    return dx


def bce_logits(logits: Tensor, target: Tensor, c: int, gscale: float, want_grad: bool):
    """-> (recon = sigmoid(logits), sum of BCE(recon, target) as a device scalar, dlogits or None)."""
    pixels = logits.numel() // logits.shape[-1]
    if target.shape != logits.shape or target.dtype != torch.float32:
        raise _lib.McgenError('bce_logits: target must be fp32 in the logits\' NHWC shape')
    blocks = max(1, min(1024, (logits.numel() + 255) // 256))
    part = torch.empty(blocks, dtype=torch.float32, device=logits.device)
    recon = torch.empty_like(logits)
    dl = torch.empty_like(logits) if want_grad else None
    check(_lib.load().mcgen_bce_logits(_p(logits), _f32(target), _p(recon), _p(dl), _f32(part), blocks, float(gscale),
                                       _dt(logits.dtype), pixels, c, logits.shape[-1], _stream()), 'bce_logits')
    return recon, part.double().sum().float(), dl


def cross_entropy(logits: Tensor, target: Tensor, c: int, want_grad: bool):
    """-> (loss_rows [pixels] fp32, dlogits or None); dlogits is the gradient of the MEAN loss."""
    pixels = logits.numel() // logits.shape[-1]
    rows = torch.empty(pixels, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    if target.dtype != torch.int64 or target.numel() != pixels:
        raise _lib.McgenError('cross_entropy: target must be int64 with one entry per pixel')
    check(_lib.load().mcgen_cross_entropy(_p(logits), target.contiguous().data_ptr(), _f32(rows), _p(dl), 1.0 / pixels,
                                          _dt(logits.dtype), pixels, c, logits.shape[-1], _stream()), 'cross_entropy')
    return rows, dl


def argmin_channels(x: Tensor, c: int) -> Tensor:
    """idx[...] = argmin over the first c channels of x[..., Cp] (int64)."""
    pixels = x.numel() // x.shape[-1]
    idx = torch.empty(x.shape[:-1], dtype=torch.int64, device=x.device)
    check(_lib.load().mcgen_argmin_channels(_p(x), idx.data_ptr(), _dt(x.dtype), pixels, c, x.shape[-1], _stream()), 'argmin_channels')
    return idx


def vq_step(feat: Tensor, idx: Tensor, embedding: Tensor, d: int, dtype: torch.dtype, coef: float = 0.0,
            want_grad: bool = False, train: bool = False, cluster_size: Optional[Tensor] = None,
            embedding_mean: Optional[Tensor] = None, decay: float = 0.99, eps: float = 1e-5, want_counts: bool = False):
    """The training step of VectorQuantization.forward (modules.py:18-43) after the nearest-code search.
    `feat` fp32 [..., Fp] (first d channels), `idx` int64 [...] the chosen codes, `embedding` [D, K] fp32.
    -> (q [..., d] in `dtype` = E[:, idx] gathered BEFORE the update, g = coef * (f - q) or None, diff = mean((q - f)^2)
    as a device scalar, counts [K] fp32 or None).  train: the EMA update of cluster_size / embedding_mean / embedding,
    in place, deterministic (mcgen_vq_stats + mcgen_vq_update)."""
    pixels = idx.numel()
    k = embedding.shape[1]
    if feat.dtype != torch.float32 or feat.numel() != pixels * feat.shape[-1] or idx.dtype != torch.int64:
        raise _lib.McgenError('vq_step: fp32 features with one int64 code per pixel expected')
    lib = _lib.load()
    chunks = lib.mcgen_vq_chunks(pixels)
    dev = feat.device
    q = torch.empty((*idx.shape, d), dtype=dtype, device=dev)
    g = torch.empty_like(q) if want_grad else None
    dpart = torch.empty(chunks, dtype=torch.float32, device=dev)
    slab = torch.empty((chunks, d, k), dtype=torch.float32, device=dev) if train else None
    cslab = torch.empty((chunks, k), dtype=torch.float32, device=dev) if train else None
    idx = idx.contiguous()
    check(lib.mcgen_vq_stats(_f32(feat), idx.data_ptr(), _f32(embedding), _p(q), _p(g), _f32(slab), _f32(cslab), _f32(dpart),
                             float(coef), _dt(dtype), pixels, d, feat.shape[-1], k, int(train), _stream()), 'vq_stats')
    diff = torch.empty((), dtype=torch.float32, device=dev)
    counts = torch.empty(k, dtype=torch.float32, device=dev) if (train and want_counts) else None
    cs = torch.empty(k, dtype=torch.float32, device=dev) if train else None
    check(lib.mcgen_vq_update(_f32(slab), _f32(cslab), _f32(dpart), pixels, d, k, float(decay), float(1.0 - decay), float(eps),
                              _f32(cluster_size) if train else None, _f32(embedding_mean) if train else None,
                              _f32(embedding) if train else None, _f32(counts), _f32(cs), _f32(diff), int(train), _stream()),
          'vq_update')
    return q, g, diff, counts


def mse_tanh(x: Tensor, target: Tensor, c: int, gscale: float, want_grad: bool):
    """-> (decoded = tanh(x), sum of (decoded - target)^2 as a device scalar, dx = gscale * (decoded - target) *
    (1 - decoded^2) or None).  `target` fp32 in x's NHWC shape."""
    pixels = x.numel() // x.shape[-1]
    if target.shape != x.shape or target.dtype != torch.float32:
        raise _lib.McgenError('mse_tanh: target must be fp32 in x\'s NHWC shape')
    blocks = max(1, min(1024, (x.numel() // 8 + 255) // 256))
    part = torch.empty(blocks, dtype=torch.float32, device=x.device)
    dec = torch.empty_like(x)
    dx = torch.empty_like(x) if want_grad else None
    check(_lib.load().mcgen_mse_tanh(_p(x), _f32(target), _p(dec), _p(dx), _f32(part), blocks, float(gscale), _dt(x.dtype), pixels,
                                     c, x.shape[-1], _stream()), 'mse_tanh')
    return dec, part.double().sum().float(), dx


def prep_weight_ex(w: Tensor, dtype: torch.dtype, ksize: Optional[int] = None, *, kh0: int = 0, kw0: int = 0,
                   transpose: bool = False, row_scale: Optional[Tensor] = None, col_scale: Optional[Tensor] = None,
                   rows_img: Optional[int] = None, k_img: Optional[int] = None, wscale: float = 1.0) -> Tensor:
    """Weight image straight from a (possibly strided / narrower) master tensor [Cout, Cin(, KH, KW)]: the source taps
    sit at (kh0, kw0) of the ksize x ksize image, row_scale[co] / col_scale[ci] scale the SOURCE, `transpose` builds the
    input-gradient image, rows_img / k_img widen the image with zeros (see mcgen_prep_weight_ex)."""
    if w.dtype != torch.float32 or not w.is_cuda:
        raise _lib.McgenError('prep_weight_ex: float32 device tensor expected')
    cout, cin = w.shape[0], w.shape[1]
    kh, kw = (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, 1)
    st = w.stride()
    s_kh, s_kw = (st[2], st[3]) if w.dim() == 4 else (0, 0)
    ks = ksize if ksize is not None else kh
    rows = rows_img if rows_img is not None else (cin if transpose else cout)
    kk = k_img if k_img is not None else (cout if transpose else cin)
    n = weight_image_elems(kk if transpose else rows, rows if transpose else kk, ks, transpose)
    out = torch.empty(n, dtype=dtype, device=w.device)
    check(_lib.load().mcgen_prep_weight_ex(w.data_ptr(), st[0], st[1], s_kh, s_kw, cout, cin, kh, kw, kh0, kw0, ks, int(transpose),
                                           rows, kk, _f32(row_scale), _f32(col_scale), float(wscale), _p(out), _dt(dtype), _stream()),
          'prep_weight_ex')
    return out


def prep_weight_ex_many(jobs, dtype: torch.dtype):
    """Several prep_weight_ex images in ceil(n / MCGEN_PREPEX_MAX) = ceil(n / 32) launches.  `jobs`: list of (w, kwargs) with the keyword arguments of
    prep_weight_ex (ksize, kh0, kw0, transpose, row_scale, col_scale, rows_img, k_img, wscale).  Returns the images."""
    if not jobs:
        return []
    arr = (_lib.PrepEx * len(jobs))()
    outs, keep = [], []
    for a, (w, kw) in zip(arr, jobs):
        if w.dtype != torch.float32 or not w.is_cuda:
            raise _lib.McgenError('prep_weight_ex_many: float32 device tensors expected')
        cout, cin = w.shape[0], w.shape[1]
        kh, kwid = (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, 1)
        st = w.stride()
        transpose = bool(kw.get('transpose', False))
        ks = kw.get('ksize') or kh
        rows = kw.get('rows_img') or (cin if transpose else cout)
        kk = kw.get('k_img') or (cout if transpose else cin)
        out = kw.get('out')                                 # (a caller-owned slice: K-concatenated images without a torch.cat)
        if out is None:
            out = torch.empty(weight_image_elems(rows, kk, ks, False), dtype=dtype, device=w.device)
        elif out.numel() != weight_image_elems(rows, kk, ks, False) or out.dtype != dtype or not out.is_contiguous():
            raise _lib.McgenError('prep_weight_ex_many: `out` must be a contiguous image-sized tensor of the compute dtype')
        a.w, a.s_co, a.s_ci = w.data_ptr(), st[0], st[1]
        a.s_kh, a.s_kw = (st[2], st[3]) if w.dim() == 4 else (0, 0)
        a.Cout, a.Cin, a.KH, a.KW = cout, cin, kh, kwid
        a.kh0, a.kw0, a.ksize, a.transpose = kw.get('kh0', 0), kw.get('kw0', 0), ks, int(transpose)
        a.rows_img, a.k_img = rows, kk
        rs, cs = kw.get('row_scale'), kw.get('col_scale')
        a.row_scale, a.col_scale, a.image, a.wscale = _f32(rs), _f32(cs), _p(out), float(kw.get('wscale', 1.0))
        outs.append(out)
        keep += [w, rs, cs]
    check(_lib.load().mcgen_prep_weight_ex_batch(arr, len(jobs), _dt(dtype), _stream()), 'prep_weight_ex_batch')
    return outs


# ---- MCPixelCNN incremental sampling (pixelcnn_sampler.py) ------------------------------------------------------------
def px_sample_row(P: '_lib.PxSample', i: int, dtype: torch.dtype):
    """Row launch i: vertical stacks, gate_v and vert_to_horiz of row i for every layer (mcgen_px_sample_row)."""
    check(_lib.load().mcgen_px_sample_row(C.byref(P), i, _dt(dtype), _stream()), 'px_sample_row')


def px_sample_col(P: '_lib.PxSample', i: int, j: int, dtype: torch.dtype):
    """Column launch (i, j): horizontal path, head, softmax and draw of position (i, j) (mcgen_px_sample_col)."""
    check(_lib.load().mcgen_px_sample_col(C.byref(P), i, j, _dt(dtype), _stream()), 'px_sample_col')


# ---- CGAN label embedding (cgan_engine.py) ------------------------------------------------------------------------------
def _labels64(label: Tensor) -> Tensor:
    if label.dtype != torch.int64 or label.dim() != 1:
        raise _lib.McgenError(f'labels must be a 1-d int64 tensor, got {label.dtype} {tuple(label.shape)}')
    return label.contiguous()


def cgan_gen_input(z: Tensor, w: Tensor, label: Tensor, dtype: torch.dtype) -> Tensor:
    """[N, 1, 1, pad8(L + E)] in `dtype`: the generator Linear's input rows z (+) W[:, label] (cgan.py:57-59), w = [E, M]."""
    n, lat = z.shape
    e, m = w.shape
    cp = pad8(lat + e)
    out = torch.empty((n, 1, 1, cp), dtype=dtype, device=z.device)
    check(_lib.load().mcgen_cgan_gen_input(_f32(z.contiguous()), _f32(w), _p(_labels64(label)), _p(out), _dt(dtype), n, lat, e, m,
                                           cp, _stream()), 'cgan_gen_input')
    return out


def cgan_dis_input(img: Tensor, cimg: int, w: Tensor, sigma: Tensor, label: Tensor) -> Tensor:
    """[N, H, W, pad8(cimg + E)] in img's dtype: the image (NHWC, `cimg` true channels) (+) (W / sigma)[:, label] broadcast
    over the pixels (cgan.py:166-169)."""
    n, h, wd, cpi = img.shape
    e, m = w.shape
    cp = pad8(cimg + e)
    out = torch.empty((n, h, wd, cp), dtype=img.dtype, device=img.device)
    check(_lib.load().mcgen_cgan_dis_input(_p(img), _f32(w), _f32(sigma), _p(_labels64(label)), _p(out), _dt(img.dtype), n, h * wd,
                                           cimg, cpi, e, m, cp, _stream()), 'cgan_dis_input')
    return out


def cgan_embed_bwd(de: Tensor, label: Tensor, dw: Tensor, accumulate: bool = False):
    """dw [E, M] (+)= sum over samples n with label_n == m of de[n] (ascending n; absent modes 0)."""
    n, e = de.shape
    m = dw.shape[1]
    check(_lib.load().mcgen_cgan_embed_bwd(_f32(de), de.stride(0), _p(_labels64(label)), _f32(dw), n, e, m, int(accumulate),
                                           _stream()), 'cgan_embed_bwd')


def cgan_lin_dembed(dlin: Tensor, w_lin: Tensor, col0: int, e: int) -> Tensor:
    """[N, E] fp32: the Linear's input gradient at columns col0 .. col0 + E from its output gradient dlin ([N, 4, 4, C0], the
    generator's row_perm-16 layout) and the fp32 master weight [16 C0, in_features]."""
    n = dlin.shape[0]
    c0 = dlin.shape[-1]
    out = torch.empty((n, e), dtype=torch.float32, device=dlin.device)
    check(_lib.load().mcgen_cgan_lin_dembed(_p(dlin), _f32(w_lin), _f32(out), _dt(dlin.dtype), n, c0, w_lin.shape[1], col0, e,
                                            _stream()), 'cgan_lin_dembed')
    return out


def cgan_dis_dembed(dc1: Tensor, c: int, dy: Tensor, w1: Tensor, wsc: Tensor, sigma1: Tensor, sigma_sc: Tensor, cimg: int,
                    e: int) -> Tensor:
    """[N, E] fp32: the discriminator embedding's input gradient through the FirstDisResBlock from conv1's output gradient
    dc1 [N, H, W, Cp] (per-image window sums) and the block's output gradient dy [N, H/2, W/2, Cp'] (the shortcut's sum);
    w1 / wsc the fp32 weight_orig of conv1 / the 1x1 shortcut, sigma1 / sigma_sc their device sigmas.  Two launches."""
    n, h, wd, cp = dc1.shape
    part = torch.empty((n, h, 3, c), dtype=torch.float32, device=dc1.device)
    check(_lib.load().mcgen_cgan_dis_window_sums(_p(dc1), _f32(part), _dt(dc1.dtype), n, h, wd, c, cp, _stream()),
          'cgan_dis_window_sums')
    out = torch.empty((n, e), dtype=torch.float32, device=dc1.device)
    check(_lib.load().mcgen_cgan_dis_dembed(_f32(part), _p(dy), _f32(w1), _f32(wsc), _f32(sigma1), _f32(sigma_sc), _f32(out),
                                            _dt(dy.dtype), n, h, c, w1.shape[1], cimg, e, dy.shape[1] * dy.shape[2], dy.shape[-1],
                                            _stream()), 'cgan_dis_dembed')
    return out


# ---- CPixelCNN conditional gates (cpixelcnn_engine.py) -------------------------------------------------------------------
def _cgate_jobs(items, fwd: bool):
    arr = (_lib.CGate * len(items))()
    outs = []
    for d, it in zip(arr, items):
        s, table, label = it[:3]
        n, h, w, c2 = s.shape
        m = table.shape[0]
        if table.dtype != torch.float32 or tuple(table.shape) != (m, c2) or not table.is_contiguous():
            raise _lib.McgenError(f'cpx gate: the embedding table must be contiguous fp32 [M, {c2}], got {table.dtype} {tuple(table.shape)}')
        d.s, d.table, d.label = _p(s), _p(table), _p(_labels64(label))
        d.N, d.HW, d.C, d.M = n, h * w, c2 // 2, m
        if fwd:
            out = torch.empty((n, h, w, c2 // 2), dtype=s.dtype, device=s.device)
            d.scale, d.shift, d.out = _f32(it[3]), _f32(it[4]), _p(out)
        else:
            blocks = max(1, min(256, (n * h * w) // 16))
            out = torch.empty((blocks, 2, c2 // 2), dtype=torch.float32, device=s.device)
            d.partials, d.blocks = _p(out), blocks
        outs.append(out)
    return arr, outs


def cpx_gate_stats(items):
    """items = [(s [N, H, W, 2C], table fp32 [M, 2C], label int64 [N])] -> [partials [blocks, 2, C]]: the BatchNorm sums of
    s[..., :C] + table[label] per gate, in the layout bn_finalize / bn_finalize_batch read (mcgen_cpx_gate_stats, one launch)."""
    arr, outs = _cgate_jobs(items, False)
    check(_lib.load().mcgen_cpx_gate_stats(arr, len(items), _dt(items[0][0].dtype), _stream()), 'cpx_gate_stats')
    return outs


def cpx_gated_fwd(items):
    """items = [(s, table, label, scale, shift)] -> [relu((a + e_a) * scale + shift) * sigmoid(b + e_b)], one launch."""
    arr, outs = _cgate_jobs(items, True)
    check(_lib.load().mcgen_cpx_gated_fwd(arr, len(items), _dt(items[0][0].dtype), _stream()), 'cpx_gated_fwd')
    return outs


def cpx_gated_bwd(s: Tensor, table: Tensor, label: Tensor, scale, shift, mean, rstd, g: Tensor, dgamma: Tensor, dbeta: Tensor):
    """Backward of cpx_gated_fwd through the batch statistics -> (ds [.., 2C], per-image channel sums of ds [N, 2C] fp32);
    fills dgamma / dbeta."""
    n, h, w, c2 = s.shape
    c = c2 // 2
    pixels = n * h * w
    blocks = max(1, min(256, pixels // 16))
    lab = _labels64(label)
    ds = torch.empty_like(s)
    part = torch.empty((blocks, 2, c), dtype=torch.float32, device=s.device)
    dsum = torch.empty((n, c2), dtype=torch.float32, device=s.device)
    lib = _lib.load()
    check(lib.mcgen_cpx_gated_bwd_stats(_p(s), _f32(table), _p(lab), table.shape[0], _f32(scale), _f32(shift), _f32(mean), _f32(rstd),
                                        _p(g), _p(ds), _f32(part), blocks, _dt(s.dtype), n, h * w, c, _stream()), 'cpx_gated_bwd_stats')
    sums = _bwd_sums(part, c, dgamma, dbeta)
    check(lib.mcgen_cpx_gated_bwd_apply(_p(ds), _p(s), _f32(table), _p(lab), table.shape[0], _f32(sums), _f32(scale), _f32(mean),
                                        _f32(rstd), float(pixels), _f32(dsum), _dt(s.dtype), n, h * w, c, _stream()),
          'cpx_gated_bwd_apply')
    return ds, dsum


def cpx_embed_bwd(dsum_v: Optional[Tensor], dsum_h: Tensor, label: Tensor, de: Tensor):
    """de [M, 2C] = sum over samples n with label_n == m of dsum_v[n] + dsum_h[n] (ascending n; absent modes 0)."""
    n, c2 = dsum_h.shape
    check(_lib.load().mcgen_cpx_embed_bwd(_f32(dsum_v), _f32(dsum_h), _p(_labels64(label)), _f32(de), n, c2, de.shape[0], _stream()),
          'cpx_embed_bwd')


def cpx_code_embed_bwd(dx: Tensor, codes: Tensor, de: Tensor):
    """de [K, C] = sum over pixels (ascending) with codes == k of dx[..., :C]: the code embedding's gradient, fixed order
    (mcgen_cpx_code_embed_bwd).  dx [N, H, W, Cp] in the compute dtype, codes int64 [N, H, W]."""
    cp = dx.shape[-1]
    k, c = de.shape
    if codes.dtype != torch.int64 or codes.numel() * cp != dx.numel():
        raise _lib.McgenError('cpx_code_embed_bwd: int64 codes, one per pixel of dx')
    check(_lib.load().mcgen_cpx_code_embed_bwd(_p(dx), cp, _p(codes.contiguous()), _f32(de), codes.numel(), k, c, _dt(dx.dtype),
                                               _stream()), 'cpx_code_embed_bwd')


def cpx_gather_rows(tables: Tensor, label: Tensor) -> Tensor:
    """tables fp32 [L, M, 2C] -> [L, N, 2C]: each layer's row of each sample's (clamped) label."""
    nl, m, c2 = tables.shape
    n = label.numel()
    out = torch.empty((nl, n, c2), dtype=torch.float32, device=tables.device)
    check(_lib.load().mcgen_cpx_gather_rows(_f32(tables.contiguous()), _p(_labels64(label)), _f32(out), nl, n, c2, m, _stream()),
          'cpx_gather_rows')
    return out


def cpx_sample_row(P: '_lib.PxSample', i: int, dtype: torch.dtype):
    """px_sample_row for ConditionalGatedPixelCNN: P.mc holds the per-sample rows [L][N][2C] (mcgen_cpx_sample_row)."""
    check(_lib.load().mcgen_cpx_sample_row(C.byref(P), i, _dt(dtype), _stream()), 'cpx_sample_row')


def cpx_sample_col(P: '_lib.PxSample', i: int, j: int, dtype: torch.dtype):
    """px_sample_col for ConditionalGatedPixelCNN (mcgen_cpx_sample_col)."""
    check(_lib.load().mcgen_cpx_sample_col(C.byref(P), i, j, _dt(dtype), _stream()), 'cpx_sample_col')


# ---- CVAE label embedding (cvae_engine.py) -------------------------------------------------------------------------------
def _table(w: Tensor, what: str) -> Tensor:
    if w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous():
        raise _lib.McgenError(f'{what}: the embedding table must be contiguous fp32 [E, M], got {w.dtype} {tuple(w.shape)}')
    return w


def cvae_enc_input(img: Tensor, w: Tensor, label: Tensor, dtype: torch.dtype) -> Tensor:
    """[N, H, W, pad8(C + E)] in `dtype` from the NCHW fp32 image in (-1, 1): (img + 1) / 2 (+) W[:, label] broadcast over the
    pixels (cvae.py:58-62, 133), w = [E, M].  One launch (mcgen_cvae_enc_input)."""
    n, c, h, wd = img.shape
    e, m = _table(w, 'cvae_enc_input').shape
    if label.numel() != n:
        raise _lib.McgenError(f'cvae_enc_input: {label.numel()} labels for {n} images')
    cp = pad8(c + e)
    out = torch.empty((n, h, wd, cp), dtype=dtype, device=img.device)
    check(_lib.load().mcgen_cvae_enc_input(_f32(img), _f32(w), _p(_labels64(label)), _p(out), _dt(dtype), n, h * wd, c, e, m, cp,
                                           _stream()), 'cvae_enc_input')
    return out


def cvae_enc_dembed(d_h: Tensor, w_conv: Tensor, cimg: int, e: int) -> Tensor:
    """[N, E] fp32: the encoder embedding's input gradient through Conv2d(cimg + E, C, 4, 2, 1) from the convolution's output
    gradient d_h [N, Ho, Wo, Cp] alone (per-image window sums; no input gradient of the convolution); w_conv the fp32 weight
    [C, cimg + E, 4, 4].  Two launches (mcgen_cgan_dis_window_sums + mcgen_cvae_enc_dembed)."""
    n, h, wd, cp = d_h.shape
    c, cin = w_conv.shape[0], w_conv.shape[1]
    if tuple(w_conv.shape[2:]) != (4, 4) or not w_conv.is_contiguous() or c > cp:
        raise _lib.McgenError(f'cvae_enc_dembed: expected a contiguous [C <= {cp}, Cin, 4, 4] weight, got {tuple(w_conv.shape)}')
    part = torch.empty((n, h, 3, c), dtype=torch.float32, device=d_h.device)
    check(_lib.load().mcgen_cgan_dis_window_sums(_p(d_h), _f32(part), _dt(d_h.dtype), n, h, wd, c, cp, _stream()),
          'cgan_dis_window_sums')
    out = torch.empty((n, e), dtype=torch.float32, device=d_h.device)
    check(_lib.load().mcgen_cvae_enc_dembed(_f32(part), _f32(w_conv), _f32(out), n, h, c, cin, cimg, e, _stream()), 'cvae_enc_dembed')
    return out


def cvae_latent_fwd(ml: Tensor, eps: Optional[Tensor], w: Tensor, label: Tensor, latent: int):
    """The latent step in one host call: ml [N, >= 2L] (compute dtype; mu | logvar head output), eps [N, L] fp32 or None
    (evaluation: z = mu), w = [E, M] -> (mu, logvar [N, L] fp32, zrow [N, 1, 1, pad8(L + E)] in ml's dtype =
    z (+) W[:, label], kld device scalar [1] = 0.5 sum(mu^2 + exp(logvar) - 1 - logvar), summed per sample then over n
    ascending)."""
    n, ldm = ml.shape
    e, m = _table(w, 'cvae_latent_fwd').shape
    if label.numel() != n or (eps is not None and tuple(eps.shape) != (n, latent)):
        raise _lib.McgenError('cvae_latent_fwd: one label and one eps row [L] per sample')
    cp = pad8(latent + e)
    dev = ml.device
    mu = torch.empty((n, latent), dtype=torch.float32, device=dev)
    logvar = torch.empty_like(mu)
    zrow = torch.empty((n, 1, 1, cp), dtype=ml.dtype, device=dev)
    kl = torch.empty(n, dtype=torch.float32, device=dev)
    kld = torch.empty(1, dtype=torch.float32, device=dev)
    check(_lib.load().mcgen_cvae_latent_fwd(_p(ml), ldm, _f32(eps), _f32(w), _p(_labels64(label)), _f32(mu), _f32(logvar), _p(zrow),
                                            _f32(kl), _f32(kld), _dt(ml.dtype), n, latent, e, m, cp, _stream()), 'cvae_latent_fwd')
    return mu, logvar, zrow, kld


def cvae_latent_bwd(dzrow: Tensor, mu: Tensor, logvar: Tensor, eps: Tensor, inv_numel: float, e: int):
    """dzrow [N, >= L + E] (compute dtype; the decoder Linear's input gradient) -> (dml [N, 1, 1, pad8(2L)] in its dtype =
    [dmu | dlogvar | 0] for the head's weight gradient, de [N, E] fp32 = columns [L, L + E): the decoder embedding's dE)."""
    n, ldz = dzrow.shape
    latent = mu.shape[1]
    if tuple(logvar.shape) != (n, latent) or tuple(eps.shape) != (n, latent) or mu.shape[0] != n:
        raise _lib.McgenError('cvae_latent_bwd: mu, logvar and eps must be [N, L]')
    cq = pad8(2 * latent)
    dml = torch.empty((n, 1, 1, cq), dtype=dzrow.dtype, device=dzrow.device)
    de = torch.empty((n, e), dtype=torch.float32, device=dzrow.device)
    check(_lib.load().mcgen_cvae_latent_bwd(_p(dzrow), ldz, _f32(mu), _f32(logvar), _f32(eps), float(inv_numel), _p(dml), _f32(de),
                                            _dt(dzrow.dtype), n, latent, e, cq, _stream()), 'cvae_latent_bwd')
    return dml, de


# ---- CGlow label-conditioned prior (glow_engine.py: CGlowEngine) --------------------------------------------------------
def _cglow_params(b_p: Tensor, s_p: Tensor, w_e: Tensor, b_e: Tensor, s_e: Tensor, label: Tensor, what: str):
    """(C2, M) of the last block's ZeroConv2d pair: prior bias / scale, embedding weight [C2, M(, 1, 1)] / bias / scale, all
    contiguous fp32 with C2 entries per vector."""
    c2 = b_p.numel()
    if w_e.dim() not in (2, 4) or w_e.shape[0] != c2 or w_e.numel() != c2 * w_e.shape[1] or c2 % 2:
        raise _lib.McgenError(f'{what}: the embedding weight must be [{c2}, M(, 1, 1)] with an even channel count, got {tuple(w_e.shape)}')
    if any(t.numel() != c2 for t in (s_p, b_e, s_e)):
        raise _lib.McgenError(f'{what}: prior / embedding biases and scales must hold {c2} entries each')
    if label.dim() != 1:
        raise _lib.McgenError(f'{what}: labels must be a vector')
    return c2, w_e.shape[1]


def cglow_prior(b_p: Tensor, s_p: Tensor, w_e: Tensor, b_e: Tensor, s_e: Tensor, label: Tensor, h: int, w: int,
                dtype: torch.dtype) -> Tensor:
    """[N, h, w, pad8(C2)] in `dtype`: prior(zeros) + embedding(one_hot(label)) of CGlow's last block (cglow.py:231-235),
    b_p exp(3 s_p) + (w_e[:, label] + b_e) exp(3 s_e) at every pixel, pad channels zero.  One launch (mcgen_cglow_prior)."""
    c2, m = _cglow_params(b_p, s_p, w_e, b_e, s_e, label, 'cglow_prior')
    n, cp = label.numel(), pad8(c2)
    out = torch.empty((n, h, w, cp), dtype=dtype, device=b_p.device)
    check(_lib.load().mcgen_cglow_prior(_f32(b_p), _f32(s_p), _f32(w_e), _f32(b_e), _f32(s_e), _p(_labels64(label)), _p(out),
                                        _dt(dtype), n, h * w, c2, m, cp, _stream()), 'cglow_prior')
    return out


def cglow_prior_bwd(dprior: Tensor, b_p: Tensor, s_p: Tensor, w_e: Tensor, b_e: Tensor, s_e: Tensor, label: Tensor,
                    db_p: Tensor, ds_p: Tensor, dw_p: Optional[Tensor], dw_e: Tensor, db_e: Tensor, ds_e: Tensor):
    """Backward of cglow_prior from dprior [N, H, W, Cp] (gaussian_logp_bwd's): overwrites the gradients of the prior's bias /
    scale, the embedding's weight / bias / scale, and zeroes dw_p (prior.conv.weight reads only zeros).  Fixed summation order
    (pixels, then samples, ascending); three launches (mcgen_cglow_prior_bwd)."""
    c2, m = _cglow_params(b_p, s_p, w_e, b_e, s_e, label, 'cglow_prior_bwd')
    n, cp = dprior.shape[0], dprior.shape[-1]
    if label.numel() != n or cp < c2:
        raise _lib.McgenError(f'cglow_prior_bwd: {label.numel()} labels, {c2} channels for a gradient of shape {tuple(dprior.shape)}')
    if dw_e.numel() != w_e.numel() or any(t.numel() != c2 for t in (db_p, ds_p, db_e, ds_e)):
        raise _lib.McgenError('cglow_prior_bwd: every gradient must have its parameter\'s size')
    ws = torch.empty(2 * n * c2, dtype=torch.float32, device=dprior.device)
    check(_lib.load().mcgen_cglow_prior_bwd(_p(dprior), _f32(b_p), _f32(s_p), _f32(w_e), _f32(b_e), _f32(s_e), _p(_labels64(label)),
                                            _f32(ws), _f32(db_p), _f32(ds_p), _f32(dw_p), 0 if dw_p is None else dw_p.numel(),
                                            _f32(dw_e), _f32(db_e), _f32(ds_e), _dt(dprior.dtype), n, dprior.numel() // (n * cp),
                                            c2, m, cp, _stream()), 'cglow_prior_bwd')


# ---- Davies-Bouldin index (metrics.davies_bouldin) ------------------------------------------------------------------------
def _i64(t: Tensor, what: str) -> int:
    if t.dtype != torch.int64:
        raise _lib.McgenError(f'{what}: expected int64, got {t.dtype}')
    return _p(t)


def _f64(t: Tensor) -> int:
    if t.dtype != torch.float64:
        raise _lib.McgenError(f'expected float64, got {t.dtype}')
    return _p(t)


def dbi_centroids(x: Tensor, order: Tensor, offset: Tensor) -> Tensor:
    """fp64 [K, D]: the mean of the rows of x [N, D] fp32 in each segment offset[k] .. offset[k + 1] of `order` (row ids sorted
    by cluster).  One launch (mcgen_dbi_centroids)."""
    n, d = x.shape
    k = offset.numel() - 1
    if order.numel() != n or k < 1:
        raise _lib.McgenError(f'dbi_centroids: {order.numel()} sorted row ids and {k} clusters for {n} rows')
    cent = torch.empty((k, d), dtype=torch.float64, device=x.device)
    check(_lib.load().mcgen_dbi_centroids(_f32(x), _i64(order, 'dbi_centroids'), _i64(offset, 'dbi_centroids'), _f64(cent), n, d, k,
                                          _stream()), 'dbi_centroids')
    return cent


def dbi_spread(x: Tensor, order: Tensor, cluster: Tensor, offset: Tensor, cent: Tensor) -> Tensor:
    """fp64 [K]: per cluster the mean Euclidean distance of its rows to its centroid.  Two launches (mcgen_dbi_spread)."""
    n, d = x.shape
    k = cent.shape[0]
    if order.numel() != n or cluster.numel() != n or offset.numel() != k + 1 or cent.shape[1] != d:
        raise _lib.McgenError('dbi_spread: one sorted id and one cluster per row, K + 1 offsets, centroids [K, D]')
    dist = torch.empty(n, dtype=torch.float64, device=x.device)
    spread = torch.empty(k, dtype=torch.float64, device=x.device)
    check(_lib.load().mcgen_dbi_spread(_f32(x), _i64(order, 'dbi_spread'), _i64(cluster, 'dbi_spread'), _i64(offset, 'dbi_spread'),
                                       _f64(cent), _f64(dist), _f64(spread), n, d, k, _stream()), 'dbi_spread')
    return spread


def dbi_score(cent: Tensor, spread: Tensor) -> Tensor:
    """fp64 [3] on the device: (mean_k max_l (s_k + s_l) / ||c_k - c_l|| with a zero distance counting as +inf, max_k s_k,
    max_kl ||c_k - c_l||).  Two launches (mcgen_dbi_score)."""
    k, d = cent.shape
    if spread.numel() != k:
        raise _lib.McgenError(f'dbi_score: {spread.numel()} spreads for {k} centroids')
    lib = _lib.load()
    tiles = lib.mcgen_dbi_tiles(k)
    tile_ratio = torch.empty((k, tiles), dtype=torch.float64, device=cent.device)
    tile_m = torch.empty_like(tile_ratio)
    out = torch.empty(3, dtype=torch.float64, device=cent.device)
    check(lib.mcgen_dbi_score(_f64(cent), _f64(spread), _f64(tile_ratio), _f64(tile_m), _f64(out), d, k, _stream()), 'dbi_score')
    return out


# ---- per-batch evaluation metrics (evaluate.DeviceEvaluator) ---------------------------------------------------------------
def _eval_state(work: Optional[Tensor], acc: Tensor, last: Tensor, device, what: str):
    c = _lib.CONSTANTS
    for t, size, name in ((work, c['MCGEN_EVAL_WORK'], 'work'), (acc, c['MCGEN_EVAL_SLOTS'], 'acc'), (last, c['MCGEN_EVAL_SLOTS'], 'last')):
        if t is not None and (t.dtype != torch.float64 or t.dim() != 1 or t.numel() != size or t.device != device):
            raise _lib.McgenError(f'{what}: Not valid {name}: float64 [{size}] on {device} expected, got {t.dtype} {tuple(t.shape)} on {t.device}')


def _eval_slot(slot: int, what: str) -> int:
    if not -1 <= int(slot) < _lib.CONSTANTS['MCGEN_EVAL_SLOTS']:
        raise ValueError(f'{what}: Not valid slot: {slot}')
    return int(slot)


def _eval_n(n: int, what: str) -> int:
    if int(n) < 1:
        raise ValueError(f'{what}: Not valid batch size: {n}')
    return int(n)


def eval_img(out: Tensor, tgt: Tensor, n: int, work: Tensor, acc: Tensor, last: Tensor, slot_mse: int = -1, slot_bce: int = -1,
             slot_psnr: int = -1):
    """MSE, BCE (the reference's, on (x + 1) / 2) and PSNR of two equally shaped fp32 tensors from one pass over both, in
    fp64: last[slot] = value, acc[slot] += n * value for each slot that is not -1.  Two launches (mcgen_eval_img)."""
    if out.shape != tgt.shape or out.numel() < 1 or out.device != tgt.device:
        raise ValueError(f'eval_img: Not valid input: {tuple(out.shape)} on {out.device} against {tuple(tgt.shape)} on {tgt.device}')
    slots = [_eval_slot(x, 'eval_img') for x in (slot_mse, slot_bce, slot_psnr)]
    wanted = [x for x in slots if x >= 0]
    if len(set(wanted)) != len(wanted):
        raise ValueError(f'eval_img: Not valid slot: two metrics share one of {slots}')
    po, pt = _f32(out), _f32(tgt)
    _eval_state(work, acc, last, out.device, 'eval_img')
    check(_lib.load().mcgen_eval_img(po, pt, out.numel(), _eval_n(n, 'eval_img'), _f64(work), *slots, _f64(acc), _f64(last),
                                     _stream()), 'eval_img')


def eval_nll(logits: Tensor, target: Tensor, n: int, work: Tensor, acc: Tensor, last: Tensor, slot: int):
    """F.cross_entropy(logits [N, K, ...] fp32, target [N, ...] int64, 'mean') in fp64 -> last[slot], acc[slot] += n * value.
    Two launches (mcgen_eval_nll)."""
    if logits.dim() < 2 or target.shape != logits.shape[:1] + logits.shape[2:] or logits.numel() < 1 or logits.device != target.device:
        raise ValueError(f'eval_nll: Not valid input: logits {tuple(logits.shape)} on {logits.device} against targets '
                         f'{tuple(target.shape)} on {target.device}')
    pl, pt = _f32(logits), _i64(target, 'eval_nll')
    _eval_state(work, acc, last, logits.device, 'eval_nll')
    nb, k = logits.shape[0], logits.shape[1]
    check(_lib.load().mcgen_eval_nll(pl, pt, nb, k, logits.numel() // (nb * k), _eval_n(n, 'eval_nll'), _f64(work),
                                     _eval_slot(slot, 'eval_nll'), _f64(acc), _f64(last), _stream()), 'eval_nll')


def eval_accuracy(logits: Tensor, label: Tensor, n: int, work: Tensor, acc: Tensor, last: Tensor, slot: int):
    """Top-1 accuracy in percent of logits [N, C] fp32 against label [N] int64 (first maximum; a row with a NaN is a miss)
    -> last[slot], acc[slot] += n * value.  Two launches (mcgen_eval_accuracy)."""
    if logits.dim() != 2 or label.shape != logits.shape[:1] or logits.numel() < 1 or logits.device != label.device:
        raise ValueError(f'eval_accuracy: Not valid input: logits {tuple(logits.shape)} on {logits.device} against labels '
                         f'{tuple(label.shape)} on {label.device}')
    pl, pt = _f32(logits), _i64(label, 'eval_accuracy')
    _eval_state(work, acc, last, logits.device, 'eval_accuracy')
    check(_lib.load().mcgen_eval_accuracy(pl, pt, logits.shape[0], logits.shape[1], _eval_n(n, 'eval_accuracy'), _f64(work),
                                          _eval_slot(slot, 'eval_accuracy'), _f64(acc), _f64(last), _stream()), 'eval_accuracy')


def eval_scalar(value: Tensor, n: int, acc: Tensor, last: Tensor, slot: int):
    """An fp32 device scalar (a loss) as it is, NaN included -> last[slot], acc[slot] += n * value.  One launch."""
    if value.numel() != 1:
        raise ValueError(f'eval_scalar: Not valid input: one value expected, got {tuple(value.shape)}')
    pv = _f32(value)
    _eval_state(None, acc, last, value.device, 'eval_scalar')
    check(_lib.load().mcgen_eval_scalar(pv, _eval_n(n, 'eval_scalar'), _eval_slot(slot, 'eval_scalar'), _f64(acc), _f64(last),
                                        _stream()), 'eval_scalar')


# ---- streaming IS / FID accumulators (metrics.ScoreAccumulator) --------------------------------------------------------------
def _score_input(x: Tensor, what: str, least: int) -> Tuple[int, int]:
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or not x.is_cuda or not x.is_contiguous():
        raise ValueError(f'{what}: Not valid input: a contiguous float32 [n, {"C" if least == 2 else "D"}] tensor on the device expected, got '
                         f'{getattr(x, "dtype", type(x))} {tuple(getattr(x, "shape", ()))} on {getattr(x, "device", "the host")}')
    n, c = x.shape
    if n < 1 or not least <= c <= 65535:
        raise ValueError(f'{what}: Not valid input: {n} rows of {c} columns (at least 1 row, {least} to 65535 columns)')
    return n, c


def _score_state(t: Tensor, shape: Tuple[int, ...], device, what: str, name: str):
    if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != device or not t.is_contiguous():
        raise ValueError(f'{what}: Not valid {name}: contiguous float64 {list(shape)} on {device} expected, got '
                         f'{getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))} on {getattr(t, "device", "the host")}')


def _score_work(t: Tensor, need: int, device, what: str):
    if not torch.is_tensor(t) or t.dtype != torch.float64 or t.dim() != 1 or t.numel() < need or t.device != device:
        raise ValueError(f'{what}: Not valid work: float64 [>= {need}] on {device} expected, got '
                         f'{getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))} on {getattr(t, "device", "the host")}')


def score_probs_work(n: int, c: int) -> int:
    """Doubles of workspace `score_probs` needs for logits [n, c] (0 for sizes it refuses)."""
    return int(_lib.load().mcgen_score_probs_work(int(n), int(c)))


def score_moments_work(n: int, d: int) -> int:
    """Doubles of workspace `score_moments` needs for features [n, d] (0 for sizes it refuses)."""
    return int(_lib.load().mcgen_score_moments_work(int(n), int(d)))


def score_probs(logits: Tensor, work: Tensor, psum: Tensor, plogp: Tensor):
    """psum [C] += the column sums of softmax(logits [n, C] fp32), plogp [1] += sum p log p, both float64 and computed in
    float64 (a row with a NaN makes both NaN).  Two launches (mcgen_score_probs), no synchronisation."""
    n, c = _score_input(logits, 'score_probs', 2)
    _score_state(psum, (c,), logits.device, 'score_probs', 'psum')
    _score_state(plogp, (1,), logits.device, 'score_probs', 'plogp')
    _score_work(work, score_probs_work(n, c), logits.device, 'score_probs')
    check(_lib.load().mcgen_score_probs(logits.data_ptr(), n, c, work.data_ptr(), psum.data_ptr(), plogp.data_ptr(), _stream()),
          'score_probs')


def score_moments(feat: Tensor, work: Tensor, fsum: Tensor, gram: Tensor):
    """fsum [D] += the column sums of feat [n, D] fp32, gram [D, D] += feat^T feat (raw second moments on the float64 MFMA, rows
    in ascending order; bitwise symmetric), both float64.  Three launches (mcgen_score_moments), no synchronisation."""
    n, d = _score_input(feat, 'score_moments', 1)
    _score_state(fsum, (d,), feat.device, 'score_moments', 'fsum')
    _score_state(gram, (d, d), feat.device, 'score_moments', 'gram')
    _score_work(work, score_moments_work(n, d), feat.device, 'score_moments')
    check(_lib.load().mcgen_score_moments(feat.data_ptr(), n, d, work.data_ptr(), fsum.data_ptr(), gram.data_ptr(), _stream()),
          'score_moments')
