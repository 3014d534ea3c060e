"""The plan of the MCGAN generator pass: which form every launch takes and which weight images exist.

Plain Python on host facts: no tensor, no HIP call.  `GeneratorEngine` builds one plan per codebook version / dtype / flag
set; `refresh_images`, `forward` and `warm_caps` read it and decide nothing themselves.

Controllers are numbered in the engine's order: block i's mc_1 is 2 i, its mc_2 is 2 i + 1, the image head's is 2 n.
A pass is one of three KINDS:
    plain   groups == 1, or the indicator is not known to be one-hot
    gk      grouped, one-hot: activations stay compacted between launches, consumers gather weight rows (K-major images)
    pm      grouped, one-hot, labels known, few modes: consumers read their mode's own dense image instead
A kind that is switched off routes like the one before it (pm -> gk -> plain).
"""
from typing import NamedTuple, Optional, Sequence, Tuple

KINDS = ('plain', 'gk', 'pm')
LAYOUT = {'dense': 0, 'mc': 1, 'gk': 2, 'pm': 0}         # ops.conv_fused's `kmajor` (what ops.FORM_LOG records) per form
A_IMAGE = {'dense': 'w1', 'mc': 'w1k', 'gk': 'w1g', 'pm': 'w1m'}          # GeneratorEngine.img['b{i}.' + ...] per form
B_IMAGE = {'dense': 'w2s', 'gk': 'w2sk', 'pm': 'w2sm'}


class Launch(NamedTuple):
    form: str                          # conv_a: dense | mc | gk | pm;  conv_b ++ shortcut: dense | gk | pm
    image: str                         # name in GeneratorEngine.img


class BlockRoute(NamedTuple):
    a: Launch                          # conv_a
    b: Launch                          # conv_b ++ shortcut
    x_compact: bool                    # the block input arrives compacted (by this block's mc_1)
    cap_h: Optional[int]               # compacted pitch of h (by mc_2), None: dense
    y_ctrl: Optional[int]              # controller whose mask the output is compacted by (next mc_1 or the head's), None: dense
    cap_y: Optional[int]


class Route(NamedTuple):
    blocks: Tuple[BlockRoute, ...]
    head: str                          # 'head' | 'headm'

    def layouts(self):
        """ops.FORM_LOG of the pass: Linear, conv_a and conv_b ++ shortcut of every block, image head."""
        return [0] + [LAYOUT[l.form] for r in self.blocks for l in (r.a, r.b)] + [0]


class ImageJob(NamedTuple):
    """One ops.PrepJob, tensors by name: `weight` -> img[buffer][offset : offset + elems]."""
    weight: str                        # lin | head | b{i}.w1 | b{i}.w2 | b{i}.ws
    buffer: str
    offset: int
    elems: int
    row_perm: int = 1
    kmajor: bool = False
    kmap: Optional[Tuple[int, int]] = None        # (controller, mode): the cidx part of that mode's compaction record
    kcount: int = 0
    rmap: Optional[Tuple[int, int]] = None        # (controller, mode): that mode's channel permutation


class GenPlan(NamedTuple):
    plain: Route
    gk: Route
    pm: Route
    pm_enabled: bool
    buffers: Tuple[Tuple[str, int], ...]          # persistent images (compute dtype): name, elements
    jobs: Tuple[ImageJob, ...]                    # the weight-image batch, in launch-table order
    pm_controllers: Tuple[int, ...]               # whose per-image compaction records a pm pass gathers by label


def _up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def image_elems(cout: int, cin: int, ksize: int) -> int:
    """mcgen_weight_image_elems (untransposed): 32-channel chunks x taps x rows padded to 16."""
    return (_up(cin, 8) + 31) // 32 * ksize * ksize * _up(cout, 16) * 32


def image_k_elems(cout: int, cin: int, ksize: int) -> int:
    """mcgen_weight_image_k_elems: per tap one row per (padded) input channel and a zero row."""
    return ksize * ksize * (_up(cin, 8) + 1) * _up(cout, 16)


def plan_generator(lin: Tuple[int, int], blocks: Sequence[Tuple[int, int, int]], head: Tuple[int, int], bf16: bool,
                   modes: int, caps: Sequence[Optional[int]], mc: bool, gk: bool, pm: bool, pm_head: bool,
                   pm_max_modes: int) -> GenPlan:
    """lin / head: (cin, cout); blocks: (cin, cout, side) of conv_a per residual block, side = that convolution's map side;
    caps: GeneratorEngine._cap of every controller (compacted pitch or None); the last five: gan_engine's MCGEN_* flags."""
    n = len(blocks)
    caps = [c or None for c in caps]
    gk_on = gk and bf16
    pm_on = pm and gk_on and modes <= pm_max_modes
    mc_on = mc and bf16
    # from 16x16 up a tile lies inside one image; gk: one 256-channel tile holds every output channel
    gkb = [gk_on and sd >= 16 and 64 <= co <= 256 and co % 32 == 0 and ci % 8 == 0 for ci, co, sd in blocks]
    mcb = [mc_on and sd >= 16 and co >= 64 and ci % 8 == 0 and co % 8 == 0 for ci, co, sd in blocks]
    has_h = [gkb[i] and caps[2 * i + 1] is not None for i in range(n)]
    # a block's output stays compacted only if the NEXT block reads it compacted in both of its launches
    keeps = [has_h[i] and i + 1 < n and has_h[i + 1] and caps[2 * i + 2] is not None for i in range(n)]
    x_compact = [i > 0 and keeps[i - 1] for i in range(n)]
    # per-mode images: h compacted, x arriving as the shortcut / conv_a images are laid out (compacted behind a gk block,
    # else dense), and 3x3 K segments of at least 64 channels (the software-pipelined form that reads weight sets takes
    # no less) -- a block that fails this takes the gk form in a pm pass
    x_img = [i > 0 and gkb[i - 1] for i in range(n)]
    pmb = [pm_on and has_h[i] and x_img[i] == x_compact[i] and caps[2 * i + 1] >= 64 and (not x_img[i] or caps[2 * i] >= 64)
           for i in range(n)]
    # what conv_head.hip takes, behind a last block with per-mode images: 32x32 maps, <= 8 outputs, whole 32-channel chunks
    head_pm = bool(pm_on and pm_head and n and pmb[-1] and blocks[-1][2] == 32 and head[1] <= 8 and head[0] % 32 == 0
                   and caps[2 * n] is not None and caps[2 * n] >= 64)

    def y_ctrl(i, pm):
        return 2 * i + 2 if keeps[i] else 2 * n if (pm and head_pm and i == n - 1) else None

    def route(gk, pm):
        out = []
        for i in range(n):
            cap_h = caps[2 * i + 1] if gk and has_h[i] else None
            xc = gk and x_compact[i]
            y = y_ctrl(i, pm) if cap_h is not None else None
            compacted = 'pm' if pm and pmb[i] else 'gk'
            a = compacted if xc else 'mc' if mcb[i] else 'dense'
            b = compacted if cap_h is not None else 'dense'
            out.append(BlockRoute(Launch(a, f'b{i}.{A_IMAGE[a]}'), Launch(b, f'b{i}.{B_IMAGE[b]}'), xc, cap_h, y,
                                  caps[y] if y is not None else None))
        return Route(tuple(out), 'headm' if out and out[-1].y_ctrl == 2 * n else 'head')

    buffers, jobs = [], []

    def image(name, parts, sets=1):
        # one buffer of `sets` images, each the `parts` (weight, elems, job fields) back to back; jobs in set order
        per = sum(p[1] for p in parts)
        buffers.append((name, sets * per))
        for m in range(sets):
            off = m * per
            for weight, elems, kw in parts:
                kw = {k: ((v, m) if k in ('kmap', 'rmap') and v is not None else v) for k, v in kw.items()}
                jobs.append(ImageJob(weight, name, off, elems, **kw))
                off += elems

    image('lin', [('lin', image_elems(lin[1], lin[0], 1), dict(row_perm=16))])
    for i, (ci, co, _) in enumerate(blocks):
        image(f'b{i}.w1', [(f'b{i}.w1', image_elems(co, ci, 3), {})])
        image(f'b{i}.w2s', [(f'b{i}.w2', image_elems(co, co, 3), {}), (f'b{i}.ws', image_elems(co, ci, 1), {})])
    image('head', [('head', image_elems(head[1], head[0], 3), {})])
    # K-major images of the launches that read compacted activations in a gk pass (an unhinted indicator takes them with
    # pm on as well): conv_b ++ shortcut of every gk block, conv_a behind a gk block
    for i, (ci, co, _) in enumerate(blocks):
        if gkb[i]:
            k = dict(kmajor=True)
            image(f'b{i}.w2sk', [(f'b{i}.w2', image_k_elems(co, co, 3), k), (f'b{i}.ws', image_k_elems(co, ci, 1), k)])
            if x_img[i]:
                image(f'b{i}.w1g', [(f'b{i}.w1', image_k_elems(co, ci, 3), k)])
    # per-mode dense images of the same launches: for every mode the chunked image whose input channels are the mode's
    # active ones in order (kmap), zero columns up to the compacted pitch, and whose rows are in the order the launch's
    # consumer keeps them (rmap = mcgen_conv_t.yperm): h by mc_2, y by the controller that masks it
    for i, (ci, co, _) in enumerate(blocks):
        if not pmb[i]:
            continue
        cap_x, cap_h, y = caps[2 * i], caps[2 * i + 1], y_ctrl(i, True)
        sc = dict(kmap=2 * i, kcount=cap_x, rmap=y) if x_img[i] else dict(rmap=y)
        image(f'b{i}.w2sm', [(f'b{i}.w2', image_elems(co, cap_h, 3), dict(kmap=2 * i + 1, kcount=cap_h, rmap=y)),
                             (f'b{i}.ws', image_elems(co, cap_x if x_img[i] else ci, 1), sc)], modes)
        if x_img[i]:
            image(f'b{i}.w1m', [(f'b{i}.w1', image_elems(co, cap_x, 3), dict(kmap=2 * i, kcount=cap_x, rmap=2 * i + 1))], modes)
    if head_pm:
        image('headm', [('head', image_elems(head[1], caps[2 * n], 3), dict(kmap=2 * n, kcount=caps[2 * n]))], modes)
    # K-major conv_a images of the mode-compacted kernel (conv_b ++ 1x1 shortcut stays dense: one-tap K steps cost more
    # than they save)
    for i, (ci, co, _) in enumerate(blocks):
        if mcb[i]:
            image(f'b{i}.w1k', [(f'b{i}.w1', image_k_elems(co, ci, 3), dict(kmajor=True))])

    pm_route = route(gk_on, pm_on)
    need = [c for i, r in enumerate(pm_route.blocks) if r.cap_h is not None
            for c in (2 * i + 1, r.y_ctrl) if c is not None] if pm_on else []
    return GenPlan(route(False, False), route(gk_on, False), pm_route, pm_on, tuple(buffers), tuple(jobs), tuple(need))
