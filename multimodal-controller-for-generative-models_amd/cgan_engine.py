"""Fused forward/backward schedules of the CGAN generator and discriminator (reference: src/models/cgan.py).

CGAN is MCGAN without the MultimodalControllers, conditioned by a label embedding instead: W[:, label] concatenated to
the generator's latent, and (W / sigma)[:, label] -- spectrally normalised -- broadcast over the image and concatenated
to the discriminator's input.  The convolution chains are MCGAN's with every code NULL, so these engines launch the same
fused convolution / weight-gradient / BatchNorm / spectral-norm kernels as ``gan_engine.py``; the embedding adds the
kernels of ``csrc/cgan_ops.hip`` (input rows, and the embedding gradient from the Linear's output gradient or from the
first discriminator block's per-image window sums).

What MCGAN's engines do only because of the MultimodalControllers is not done here: no codes, no compacted activations,
no per-mode weight sets, no paired D(real) + D(fake) pass (its sigma-ratio trick rides in the codes).  The grouped
generator pass (several training-mode forwards with their own BatchNorm statistics as one pass) is kept.

Labels are int64 device tensors; a module-level caller that only has the one-hot indicator passes its argmax.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import dis_plan, ops
from ._lib import McgenError
from .gan_engine import (DiscriminatorEngine, FlatState, Nhwc, _LOWRES_SC_BWD, _bn_forward, _flush_counters,
                         _pending_counters, _pending_running)
from .ops import PrepJob, Seg

Tensor = torch.Tensor


def _labels(indicator: Optional[Tensor], label: Optional[Tensor]) -> Tensor:
    if label is not None:
        return label
    if indicator is None:
        raise McgenError('CGAN engines need the labels or the one-hot indicator')
    return indicator.argmax(1)


# ============================================================================================= #
#  Generator
# ============================================================================================= #
class CGeneratorEngine:
    def __init__(self, gen, dtype: torch.dtype = torch.float32):
        self.gen = gen
        self.dtype = dtype
        self.flat_p = FlatState(list(gen.parameters()))
        self._emb_slot = next(i for i, p in enumerate(self.flat_p.tensors) if p is gen.embedding.weight)
        self._img_key = None
        self.img: Dict[str, Tensor] = {}
        self._prep_fwd = self._prep_bwd = None

    def rebind(self):
        """Follow an embedding table that create() / transit() replaced: `embedding.weight` is then a new nn.Parameter
        (another object, possibly another shape), so the flat parameter set is laid out again over the live parameters."""
        if self.flat_p.tensors[self._emb_slot] is not self.gen.embedding.weight:
            self.flat_p = FlatState(list(self.gen.parameters()))

    def _layers(self):
        """(embedding, linear, [GenResBlock], head BN, head conv) of cgan.py:39-53."""
        g = self.gen
        blocks = list(g.blocks.children())
        res = [b for b in blocks if hasattr(b, 'shortcut')]
        n = len(res)
        return g.embedding, g.linear, res, blocks[n], blocks[n + 2]

    @staticmethod
    def _convs(b):
        """conv1, conv2, shortcut conv, BN1, BN2 of a GenResBlock (cgan.py:9-27)."""
        return b.conv[3], b.conv[6], b.shortcut[1], b.conv[0], b.conv[4]

    def refresh_images(self, force: bool = False):
        emb, lin, res, head_bn, head_conv = self._layers()
        ws = [lin.weight, lin.bias, head_conv.weight]
        for b in res:
            c1, c2, sc, _, _ = self._convs(b)
            ws += [c1.weight, c2.weight, sc.weight]
        key = (self.dtype, tuple((w.data_ptr(), w._version) for w in ws))
        if not force and key == self._img_key:
            return
        dt = self.dtype
        dev = lin.weight.device
        c0 = lin.out_features // 16

        def buf(name, numel, dtype):
            t = self.img.get(name)                  # persistent: a captured graph keeps reading the same addresses
            if t is None or t.numel() != numel or t.dtype != dtype or t.device != dev:
                t = torch.empty(numel, dtype=dtype, device=dev)
                self.img[name] = t
            return t

        if self._prep_fwd is None or self._prep_fwd.dtype != dt or not self._prep_fwd.valid():
            jobs = [PrepJob(lin.weight, buf('lin', ops.weight_image_elems(lin.out_features, lin.in_features, 1), dt), row_perm=16)]
            for i, b in enumerate(res):
                c1, c2, sc, _, _ = self._convs(b)
                jobs.append(PrepJob(c1.weight, buf(f'b{i}.w1', ops.weight_image_elems(c1.out_channels, c1.in_channels, 3), dt)))
                n2 = ops.weight_image_elems(c2.out_channels, c2.in_channels, 3)
                ns = ops.weight_image_elems(sc.out_channels, sc.in_channels, 1)
                cat = buf(f'b{i}.w2s', n2 + ns, dt)
                jobs += [PrepJob(c2.weight, cat[:n2]), PrepJob(sc.weight, cat[n2:])]
            jobs.append(PrepJob(head_conv.weight, buf('head', ops.weight_image_elems(head_conv.out_channels, head_conv.in_channels, 3), dt)))
            self._prep_fwd = ops.PrepBatch(jobs, dt)
        self._prep_fwd.run()
        buf('lin_bias', lin.out_features, torch.float32).view(16, c0).copy_(lin.bias.detach().view(c0, 16).t())
        self._img_key = key

    def _prep_backward_images(self):
        emb, lin, res, head_bn, head_conv = self._layers()
        dt = self.dtype
        if self._prep_bwd is None or self._prep_bwd.dtype != dt or not self._prep_bwd.valid():
            jobs = []
            self.img_t = {}

            def tbuf(name, w):
                t = torch.empty(ops.weight_image_elems(w.shape[0], w.shape[1], w.shape[2], True), dtype=dt, device=w.device)
                self.img_t[name] = t
                jobs.append(PrepJob(w, t, transpose=True))
            tbuf('head', head_conv.weight)
            for i, b in enumerate(res):
                c1, c2, sc, _, _ = self._convs(b)
                tbuf(f'b{i}.w1', c1.weight)
                tbuf(f'b{i}.w2', c2.weight)
                tbuf(f'b{i}.ws', sc.weight)
            self._prep_bwd = ops.PrepBatch(jobs, dt)
        self._prep_bwd.run()

    def warm_caps(self):
        """(MCGAN reads its compacted pitches here before a capture; CGAN has none.)"""

    def bucket_cut(self) -> int:
        return 0

    def groups_supported(self, n_total: int, groups: int) -> bool:
        """As GeneratorEngine.groups_supported: every launch's tile must lie inside one statistics group."""
        if groups <= 1:
            return True
        if n_total % groups:
            return False
        gn = n_total // groups
        emb, lin, res, head_bn, head_conv = self._layers()
        shapes = [(1, lin.out_features)]
        side = 4
        for b in res:
            side *= 2
            shapes += [(side, self._convs(b)[0].out_channels)] * 2
        shapes.append((side, head_conv.out_channels))
        return all(gn % ops.tile_images(n_total, sd, sd, co, self.dtype) == 0 for sd, co in shapes)

    # ---- forward ---------------------------------------------------------------------------------
    def forward(self, z: Tensor, indicator: Optional[Tensor], train: bool, groups: int = 1, nhwc: bool = False,
                label: Optional[Tensor] = None, **_unused):
        """cgan.py:55-62 as fused launches.  `groups` > 1 (training mode, forward only): `groups` generator forwards of
        N / groups images each, every one with its own BatchNorm batch statistics, as one pass (GANTrainer.fake_groups).
        `nhwc`: return the images as `Nhwc` instead of NCHW fp32."""
        _pending_counters.clear(); _pending_running.clear()
        self.rebind()
        self.flat_p.ensure()
        emb, lin, res, head_bn, head_conv = self._layers()
        if train and emb.weight.shape[1] != emb.in_features:
            raise ValueError(f'Not valid mode: generator.embedding holds {emb.weight.shape[1]} modes but was built for '
                             f'{emb.in_features}; after create() only evaluation-mode generation is supported')
        dt = self.dtype
        n = z.shape[0]
        if groups > 1 and not (train and self.groups_supported(n, groups)):
            raise RuntimeError(f'generator forward: {groups} statistics groups over {n} images is not supported')
        gn = n // groups if groups > 1 else 0
        ng = n // groups
        lab = _labels(indicator, label)
        self.refresh_images()
        st_mode = 1 if train else 0
        zt = ops.cgan_gen_input(z.detach(), emb.weight.detach(), lab, dt)              # [N, 1, 1, pad8(L + E)]
        c0 = lin.out_features // 16
        x0, st = ops.conv_fused([Seg(zt, ksize=1)], self.img['lin'], 16 * c0, bias=self.img['lin_bias'], stats_mode=st_mode)
        x = x0.view(n, 4, 4, c0)
        fold = 16                              # Linear output column p * C0 + c belongs to channel c
        blocks_ctx = []
        for i, b in enumerate(res):
            c1, c2, sc, bnm1, bnm2 = self._convs(b)
            s = x.shape[1]
            co = c1.out_channels
            bn1 = _bn_forward(bnm1, st, ng * s * s, train, fold, groups)
            fold = 1
            # BN -> ReLU -> Up -> conv3x3 (cgan.py:12-15)
            h, st_h = ops.conv_fused([Seg(x, scale=bn1.scale, shift=bn1.shift, ups=True, relu=True, group_n=gn)],
                                     self.img[f'b{i}.w1'], co, bias=c1.bias, stats_mode=st_mode)
            bn2 = _bn_forward(bnm2, st_h, ng * 4 * s * s, train, 1, groups)
            # BN -> ReLU -> conv3x3, plus the Up -> conv1x1 shortcut as a second K segment (cgan.py:16-24,34)
            y, st = ops.conv_fused([Seg(h, scale=bn2.scale, shift=bn2.shift, relu=True, group_n=gn), Seg(x, ksize=1, ups=True)],
                                   self.img[f'b{i}.w2s'], co, bias=c2.bias, bias2=sc.bias, stats_mode=st_mode)
            blocks_ctx.append(dict(x=x, h=h, bn1=bn1, bn2=bn2))
            x = y
        s = x.shape[1]
        bnh = _bn_forward(head_bn, st, ng * s * s, train, fold, groups)
        cimg = head_conv.out_channels
        out, _ = ops.conv_fused([Seg(x, scale=bnh.scale, shift=bnh.shift, relu=True, group_n=gn)], self.img['head'], cimg,
                                bias=head_conv.bias, tanh=True)
        ctx = {'train': train, 'n': n, 'groups': groups, 'zt': zt, 'label': lab, 'blocks': blocks_ctx, 'y': x, 'bnh': bnh,
               'out': out}
        _flush_counters()
        return (Nhwc(out, cimg) if nhwc else ops.to_nchw(out, cimg)), ctx

    # ---- backward ----------------------------------------------------------------------------------
    def backward(self, ctx, dimg, gflat: Tensor, accumulate: bool = False):
        for _ in self.backward_iter(ctx, dimg, gflat, accumulate, split=False):
            pass

    def backward_iter(self, ctx, dimg, gflat: Tensor, accumulate: bool = False, split: bool = False):
        """Writes (or adds) every generator parameter's gradient into `gflat` (laid out like ``flat_p``); one bucket,
        yielded at the end as (0, numel, True)."""
        if not ctx['train']:
            raise RuntimeError('generator backward needs a training-mode forward (batch statistics)')
        if ctx.get('groups', 1) != 1:
            raise RuntimeError('a grouped generator pass is forward-only (its images feed discriminator updates detached)')
        emb, lin, res, head_bn, head_conv = self._layers()
        dt = self.dtype
        n = ctx['n']
        acc = accumulate
        out = ctx['out']
        self._prep_backward_images()
        dout = dimg.t if isinstance(dimg, Nhwc) else ops.to_nhwc(dimg.contiguous(), dt, out.shape[-1])
        dtn = ops.tanh_bwd(dout, out)
        y, bnh = ctx['y'], ctx['bnh']
        c_img, c = head_conv.out_channels, head_conv.in_channels
        G = lambda p: self.flat_p.view_of(gflat, p)                           # noqa: E731
        with ops.deferred_reduces():
            ops.wgrad(Seg(y, scale=bnh.scale, shift=bnh.shift, relu=True), dtn, c_img, c, G(head_conv.weight), accumulate=acc,
                      bias_grad=G(head_conv.bias))
            dz, part = ops.conv_fused([Seg(dtn)], self.img_t['head'], c, gate_x=y, gscale=bnh.scale, gshift=bnh.shift,
                                      gmean=bnh.mean, grstd=bnh.rstd, stats_mode=2)
            dy = ops.bn_backward(part, dz, y, bnh.count, bnh.scale, bnh.mean, bnh.rstd, G(head_bn.weight), G(head_bn.bias),
                                 accumulate=acc)
            for i in reversed(range(len(res))):
                bc = ctx['blocks'][i]
                x, h, bn1, bn2 = bc['x'], bc['h'], bc['bn1'], bc['bn2']
                conv1, conv2, convs, bnm1, bnm2 = self._convs(res[i])
                ci, co = conv1.in_channels, conv1.out_channels
                ops.wgrad(Seg(h, scale=bn2.scale, shift=bn2.shift, relu=True), dy, co, co, G(conv2.weight), accumulate=acc,
                          bias_grad=G(conv2.bias), bias_grad2=G(convs.bias))
                # (bf16: the shortcut's gradients at x's resolution from the 2x2-pooled dy, as GeneratorEngine.backward_iter)
                lowres = _LOWRES_SC_BWD and dt == torch.bfloat16 and dy.shape[1] >= 16
                dy_lo = ops.pool2_sum(dy) if lowres else None
                if lowres:
                    ops.wgrad(Seg(x, ksize=1), dy_lo, co, ci, G(convs.weight), accumulate=acc)
                else:
                    ops.wgrad(Seg(x, ksize=1, ups=True), dy, co, ci, G(convs.weight), accumulate=acc)
                dz2, part2 = ops.conv_fused([Seg(dy)], self.img_t[f'b{i}.w2'], co, gate_x=h, gscale=bn2.scale, gshift=bn2.shift,
                                            gmean=bn2.mean, grstd=bn2.rstd, stats_mode=2)
                dh = ops.bn_backward(part2, dz2, h, bn2.count, bn2.scale, bn2.mean, bn2.rstd, G(bnm2.weight), G(bnm2.bias),
                                     accumulate=acc)
                ops.wgrad(Seg(x, scale=bn1.scale, shift=bn1.shift, ups=True, relu=True), dh, co, ci, G(conv1.weight),
                          accumulate=acc, bias_grad=G(conv1.bias))
                if lowres:
                    dx_sc, _ = ops.conv_fused([Seg(dy_lo, ksize=1)], self.img_t[f'b{i}.ws'], ci)
                else:
                    dx_sc, _ = ops.conv_fused([Seg(dy, ksize=1)], self.img_t[f'b{i}.ws'], ci, pool=True, alpha=1.0)
                dz1, part1 = ops.conv_fused([Seg(dh)], self.img_t[f'b{i}.w1'], ci, pool=True, alpha=1.0, gate_x=x,
                                            gscale=bn1.scale, gshift=bn1.shift, gmean=bn1.mean, grstd=bn1.rstd, stats_mode=2)
                dy = ops.bn_backward(part1, dz1, x, bn1.count, bn1.scale, bn1.mean, bn1.rstd, G(bnm1.weight), G(bnm1.bias),
                                     add=dx_sc, accumulate=acc)
            # Linear: dy is [N, 4, 4, C0] == [N, 1, 1, 16 C0] in the permuted row order
            c0 = lin.out_features // 16
            ops.wgrad(Seg(ctx['zt'], ksize=1), dy.view(n, 1, 1, 16 * c0), 16 * c0, lin.in_features, G(lin.weight), row_perm=16,
                      accumulate=acc, bias_grad=G(lin.bias))
            # embedding: its columns of the Linear's input gradient, summed per label (cgan.py:58)
            de = ops.cgan_lin_dembed(dy, lin.weight.detach(), lin.in_features - emb.out_features, emb.out_features)
            ops.cgan_embed_bwd(de, ctx['label'], G(emb.weight), accumulate=acc)
        yield (0, gflat.numel(), True)


# ============================================================================================= #
#  Discriminator
# ============================================================================================= #
class CDiscriminatorEngine(DiscriminatorEngine):
    """Reuses DiscriminatorEngine's flat parameter / u-v state and its spectral-norm power iteration (the embedding is
    one more SN layer, 32 x num_mode); the forward and backward passes are CGAN's own."""

    def __init__(self, dis, dtype: torch.dtype = torch.float32):
        super().__init__(dis, dtype)
        self.emb = next(s for s in self.sn if s.m is dis.embedding)
        self.cimg = dis.data_shape[0]

    def _describe(self, sn_of):
        """As DiscriminatorEngine._describe, for cgan.py:65-153: no controllers; the first block reads image (+) embedding,
        so the generator update's input gradient covers the IMAGE channels of its conv1 / 1x1 shortcut only (plan.dimg)."""
        blocks = list(self.dis.blocks.children())
        res = [b for b in blocks if hasattr(b, 'shortcut')]
        L = lambda m: sn_of[m].layer                                          # noqa: E731
        b0 = res[0]
        facts = [dis_plan.BlockFacts(L(b0.conv[0]), L(b0.conv[2]), L(b0.shortcut[0]), True, None, None)]
        for b in res[1:]:
            facts.append(dis_plan.BlockFacts(L(b.conv[1]), L(b.conv[3]), L(b.shortcut[0]) if len(b.shortcut) > 0 else None,
                                             len(b.conv) == 5, None, None))
        tail = sn_of[blocks[len(res) + 2]]                     # ReLU, GlobalSumPooling, Linear (cgan.py:150-152)
        return facts, tail, [], dict(image_cin=self.dis.data_shape[0], one_bucket=True)

    # ---- forward ---------------------------------------------------------------------------------
    def forward(self, x_nchw, indicator: Optional[Tensor], train: bool, tail_loss: Optional[str] = None,
                label: Optional[Tensor] = None, loss_type: str = 'Hinge'):
        """cgan.py:164-170.  `tail_loss` 'g' (the generator update): the tail's launch also forms d(G loss)/d(logit) of
        `loss_type` ('Hinge' | 'BCE') and the tail's input gradient (ctx['tail']), as DiscriminatorEngine.forward."""
        sigma, uv = self._power_iter(train)
        lab = _labels(indicator, label)
        dt = self.dtype
        n = x_nchw.shape[0]
        ctx = {'n': n, 'sigma': sigma, 'uv': uv, 'blocks': [], 'pair': None, 'train': train, 'label': lab}
        self._ensure_preps()
        (self._prep_all if train else self._prep_fwd).run(sigma)
        if train:
            self._bwd_sigma = sigma
        I, S = self.img, self.sn
        img = x_nchw.t if isinstance(x_nchw, Nhwc) else ops.to_nhwc(x_nchw.detach().contiguous(), dt)
        if img.dtype != dt:
            raise RuntimeError(f'Nhwc input is {img.dtype}, the engine computes in {dt}')
        # image (+) (W / sigma)[:, label] over every pixel: one [N, H, W, pad8(C + E)] input (DESIGN.md section on CGAN)
        e = self.emb
        xin = ops.cgan_dis_input(img, self.cimg, e.m.weight_orig.detach(), sigma[e.idx:e.idx + 1], lab)
        ctx['img'], ctx['xin'], ctx['nhwc'] = img, xin, isinstance(x_nchw, Nhwc)
        b = self.plan.blocks[0]
        c1m, c2m, scm = S[b.conv1], S[b.conv2], S[b.shortcut]
        co = c1m.cout
        c1, _ = ops.conv_fused([Seg(xin)], I[b.c1], co, bias=c1m.m.bias)
        y, _ = ops.conv_fused([Seg(c1, relu=True), Seg(xin, ksize=1)], I[b.c2], co, bias=c2m.m.bias, bias2=scm.m.bias,
                              pool=True, alpha=b.alpha)
        ctx['blocks'].append({'c1': c1})
        x = y
        for b in self.plan.blocks[1:]:
            c1m, c2m = S[b.conv1], S[b.conv2]
            c1, _ = ops.conv_fused([Seg(x, relu=True)], I[b.c1], c1m.cout, bias=c1m.m.bias)
            if b.fused:
                y, _ = ops.conv_fused([Seg(c1, relu=True), Seg(x, ksize=1)], I[b.c2], c2m.cout, bias=c2m.m.bias,
                                      bias2=S[b.shortcut].m.bias, pool=b.pooled, alpha=b.alpha)
            else:
                y, _ = ops.conv_fused([Seg(c1, relu=True)], I[b.c2], c2m.cout, bias=c2m.m.bias, res=x)
            ctx['blocks'].append({'x': x, 'c1': c1})
            x = y
        # tail: ReLU -> global sum pool -> SN linear (cgan.py:150-152)
        tl = self.tail
        wl = tl.m.weight_orig.detach().view(-1)
        if tail_loss is not None and ops.dtail_hinge_ok(x):
            if tail_loss != 'g':
                raise McgenError("CGAN discriminator: tail_loss 'g' only (there is no paired pass)")
            logit, pooled_feat, dlogit, dxt = ops.dtail_loss_fused(x, None, wl, tl.m.bias, sigma[tl.idx:tl.idx + 1], 'g', loss_type)
            ctx['tail'] = (dlogit, dxt)
            ctx['loss_type'] = loss_type
        else:
            logit, pooled_feat = ops.dtail_fwd(x, None, wl, tl.m.bias, sigma[tl.idx:tl.idx + 1])
        ctx.update(xt=x, pooled=pooled_feat)
        return logit.view(n, 1), ctx

    def forward_pair(self, *a, **k):
        raise McgenError('CGAN discriminator: no paired pass (its sigma-ratio trick rides in MultimodalController codes)')

    def pair_codes(self, *a, **k):
        raise McgenError('CGAN discriminator: no MultimodalController codes')

    # ---- backward ----------------------------------------------------------------------------------
    def backward_iter(self, ctx, dlogit: Tensor, gflat: Optional[Tensor], accumulate: bool, need_input_grad: bool,
                      split: bool = False, defer_fix: bool = False):
        """dlogit [N] fp32.  Parameter gradients (w.r.t. weight_orig and the biases) are written or added into `gflat`
        (None skips them: the generator update).  One bucket, yielded at the end; returns d(input image) or None."""
        if ctx['pair'] is not None:
            raise McgenError('CGAN discriminator: no paired pass')
        fp, _ = self._ensure_flat()
        sigma, uv, lab = ctx['sigma'], ctx['uv'], ctx['label']
        want_w = gflat is not None
        gt = torch.empty_like(fp) if want_w else None          # gradients w.r.t. the NORMALISED weights land here first
        T = lambda p: self.flat_p.view_of(gt, p)               # noqa: E731
        self._ensure_preps()
        if self._bwd_sigma is not sigma:
            self._prep_bwd.run(sigma)
            self._bwd_sigma = sigma
        I, S = self.img, self.sn
        tl = self.tail
        sg_t = sigma[tl.idx:tl.idx + 1]
        wl = tl.m.weight_orig
        with ops.deferred_reduces():
            tail = ctx.get('tail')
            if tail is not None and dlogit is tail[0] and not want_w:
                dy = tail[1]
            else:
                dy = ops.dtail_bwd(dlogit, ctx['xt'], None, wl.detach().view(-1), sg_t, ctx['pooled'],
                                   T(wl).view(-1) if want_w else None, T(tl.m.bias) if want_w else None)
            blocks = self.plan.blocks
            for bi in reversed(range(1, len(blocks))):
                b, bc = blocks[bi], ctx['blocks'][bi]
                x, c1 = bc['x'], bc['c1']
                c1m, c2m = S[b.conv1], S[b.conv2]
                scm = S[b.shortcut] if b.fused else None
                if want_w:
                    ops.wgrad(Seg(c1, relu=True), dy, c2m.cout, c2m.cin, T(c2m.m.weight_orig), bias_grad=T(c2m.m.bias),
                              bias_grad2=T(scm.m.bias) if scm is not None else None, dy_ups=b.pooled, alpha=b.alpha)
                    if scm is not None:
                        ops.wgrad(Seg(x, ksize=1), dy, scm.cout, scm.cin, T(scm.m.weight_orig), dy_ups=b.pooled, alpha=b.alpha)
                dc1, _ = ops.conv_fused([Seg(dy, ups=b.pooled)], I[b.c2t], c2m.cin, gate_x=c1)
                if want_w:
                    ops.wgrad(Seg(x, relu=True), dc1, c1m.cout, c1m.cin, T(c1m.m.weight_orig), bias_grad=T(c1m.m.bias))
                if scm is not None:
                    res, _ = ops.conv_fused([Seg(dy, ksize=1, ups=b.pooled)], I[b.sct], scm.cin)
                else:
                    res = dy
                dy, _ = ops.conv_fused([Seg(dc1)], I[b.c1t], c1m.cin, gate_x=x, res=res)
            # FirstDisResBlock on the image (+) embedding input
            b = blocks[0]
            c1m, c2m, scm = S[b.conv1], S[b.conv2], S[b.shortcut]
            c1, xin = ctx['blocks'][0]['c1'], ctx['xin']
            if want_w:
                ops.wgrad(Seg(c1, relu=True), dy, c2m.cout, c2m.cin, T(c2m.m.weight_orig), bias_grad=T(c2m.m.bias),
                          bias_grad2=T(scm.m.bias), dy_ups=True, alpha=b.alpha)
                ops.wgrad(Seg(xin, ksize=1), dy, scm.cout, scm.cin, T(scm.m.weight_orig), dy_ups=True, alpha=b.alpha)
            dc1, _ = ops.conv_fused([Seg(dy, ups=True)], I[b.c2t], c2m.cin, gate_x=c1)
            if want_w:
                ops.wgrad(Seg(xin), dc1, c1m.cout, c1m.cin, T(c1m.m.weight_orig), bias_grad=T(c1m.m.bias))
                # the embedding: per-image window sums of dc1 and the plain sum of dy -- no input-gradient launch
                e = self.emb
                de = ops.cgan_dis_dembed(dc1, c1m.cout, dy, c1m.m.weight_orig.detach(), scm.m.weight_orig.detach(),
                                         sigma[c1m.idx:c1m.idx + 1], sigma[scm.idx:scm.idx + 1], self.cimg, e.cout)
                ops.cgan_embed_bwd(de, lab, T(e.m.weight_orig))
            dimg = None
            if need_input_grad:
                # only the image channels of the input gradient (the embedding's input is a parameter, not an image)
                for s in (c1m, scm):
                    self._w_cols[s.idx].copy_(s.m.weight_orig.detach()[:, :self.cimg])
                self._prep_dimg.run(sigma)
                img = ctx['img']
                dimg_t, _ = ops.conv_fused([Seg(dc1), Seg(dy, ksize=1, ups=True)], I[b.dimg], self.cimg, cy=img.shape[-1])
                dimg = Nhwc(dimg_t, self.cimg) if ctx.get('nhwc') else ops.to_nchw(dimg_t, self.cimg)
        if want_w:
            # d/d(W / sigma) -> d/d(weight_orig) with this forward's u, v, sigma; biases moved as they are
            ops.sn_grad_fix(gt, gflat, fp, uv, self._layers_dev, len(self.sn) + len(self.plain), sigma, accumulate=accumulate)
            yield (0, fp.numel(), True)
        return dimg
