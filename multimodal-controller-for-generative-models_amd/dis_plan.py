"""The plan of a GAN discriminator pass: its residual blocks as records, its weight images as named jobs.

Plain Python on host facts: no tensor, no HIP call.  Each discriminator engine describes its nn.Sequential once (`_describe`
in gan_engine.DiscriminatorEngine / cgan_engine.CDiscriminatorEngine: the only code that knows a `conv[...]` position) and
builds one plan in its constructor; the image builder, the forward and backward schedules, the code jobs of the paired pass
and the spectral-norm bucket tables read it and derive nothing themselves.

A spectrally normalised layer is named by its index in the engine's `sn` list, which is also its index in the sigma vector
of a pass.  A MultimodalController is named by its index in the engine's CodeBatch, None where a convolution input has no
controller (the raw image in MCGAN, every input in CGAN).
"""
from typing import NamedTuple, Optional, Sequence, Tuple

from .gen_plan import image_elems


class Layer(NamedTuple):
    """One spectrally normalised convolution, as the engine's _SNConv states it."""
    sn: int
    cout: int
    cin: int
    ks: int


class BlockFacts(NamedTuple):
    """What an engine reads off one residual block (block 0 is the FirstDisResBlock: it reads the image and always pools)."""
    conv1: Layer
    conv2: Layer
    shortcut: Optional[Layer]          # the 1x1 convolution, None: identity
    pooled: bool
    ctrl_x: Optional[int]              # controller on the block input (conv1 and the shortcut read through it)
    ctrl_h: Optional[int]              # controller in front of conv2


class Block(NamedTuple):
    conv1: int                         # layer indices
    conv2: int
    shortcut: Optional[int]
    pooled: bool
    alpha: float                       # the average pool's 0.25, folded into the pooled launches and their transposed images
    ctrl_x: Optional[int]
    ctrl_h: Optional[int]
    fused: bool                        # the shortcut runs as a second K segment of conv2's launch (image `c2`)
    c1: str                            # forward images
    c2: str
    sc: Optional[str]                  # the shortcut's own image (block 0 with MCGEN_D0_FUSE off)
    c2t: str                           # transposed images of the input gradients
    c1t: Optional[str]                 # None in block 0: conv1 ++ shortcut transposed share `dimg`
    sct: Optional[str]
    dimg: Optional[str]


class ImageJob(NamedTuple):
    """One ops.PrepJob, tensors by name: layer's weight_orig / sigma[sigma] * wscale -> img[buffer][offset : offset + elems]."""
    layer: int
    buffer: str
    offset: int
    elems: int
    transpose: bool
    sigma: int
    wscale: float


class DisPlan(NamedTuple):
    blocks: Tuple[Block, ...]
    tail: Tuple[int, Optional[int]]                    # (layer, controller) of the tail's Linear
    buffers: Tuple[Tuple[str, int], ...]               # persistent images (compute dtype): name, elements
    fwd: Tuple[ImageJob, ...]                          # the forward images' batch
    bwd: Tuple[ImageJob, ...]                          # the transposed images' batch (training passes run fwd + bwd as one)
    dimg: Tuple[ImageJob, ...]                         # `image_cin`: the input-gradient image's own batch, else empty
    image_cin: Optional[int]                           # the input channels `0.dimg` covers, None: all of them
    uses: Tuple[Tuple[Optional[int], int], ...]        # (controller, layer) of every convolution input, the tail's last
    bucket_cut: int                                    # first block of the late gradient bucket, 0: one bucket


def plan_discriminator(blocks: Sequence[BlockFacts], tail: Tuple[int, Optional[int]], d0_fuse: bool = True,
                       image_cin: Optional[int] = None, one_bucket: bool = False) -> DisPlan:
    """blocks: the residual blocks in order; tail: (layer, controller) of the final Linear; d0_fuse: gan_engine's
    MCGEN_D0_FUSE.  image_cin (CGAN: block 0 reads image (+) embedding): the input gradient covers the first image_cin
    input channels only, so `0.dimg` holds those columns of conv1 / the shortcut and is built by its own batch (`dimg`) from
    column copies the engine keeps; None: it holds the whole layers and rides in `bwd`.  one_bucket: the engine never
    splits its backward pass."""
    buffers, fwd, bwd, dimg = [], [], [], []

    def image(jobs, name, parts, transpose, cin=None):
        # one buffer holding the images of `parts` ((layer, wscale), ...) back to back
        off = 0
        for l, wscale in parts:
            ci = cin if cin is not None else l.cin
            n = image_elems(ci, l.cout, l.ks) if transpose else image_elems(l.cout, ci, l.ks)
            jobs.append(ImageJob(l.sn, name, off, n, transpose, l.sn, wscale))
            off += n
        buffers.append((name, off))
        return name

    out, uses = [], []
    for i, b in enumerate(blocks):
        first = i == 0
        if first and not (b.pooled and b.shortcut is not None):
            raise ValueError('the first discriminator block pools and has a 1x1 shortcut')
        c1, c2, sc = b.conv1, b.conv2, b.shortcut
        a = 0.25 if b.pooled else 1.0
        fused = sc is not None and (d0_fuse or not first)
        n_c1 = image(fwd, f'{i}.c1', [(c1, 1.0)], False)
        n_sc = n_sct = n_c1t = n_dimg = None
        if fused:
            n_c2 = image(fwd, f'{i}.c2s', [(c2, 1.0), (sc, 1.0)], False)
        else:
            if sc is not None:
                n_sc = image(fwd, f'{i}.sc', [(sc, 1.0)], False)
            n_c2 = image(fwd, f'{i}.c2', [(c2, 1.0)], False)
        if first:
            n_c2t = image(bwd, '0.c2t', [(c2, a)], True)
            n_dimg = image(bwd if image_cin is None else dimg, '0.dimg', [(c1, 1.0), (sc, a)], True, image_cin)
            uses += [(b.ctrl_x, c1.sn), (b.ctrl_x, sc.sn), (b.ctrl_h, c2.sn)]
        else:
            if sc is not None:
                n_sct = image(bwd, f'{i}.sct', [(sc, a)], True)
            n_c2t = image(bwd, f'{i}.c2t', [(c2, a)], True)
            n_c1t = image(bwd, f'{i}.c1t', [(c1, 1.0)], True)
            uses += [(b.ctrl_x, c1.sn), (b.ctrl_h, c2.sn)] + ([(b.ctrl_x, sc.sn)] if sc is not None else [])
        out.append(Block(c1.sn, c2.sn, sc.sn if sc is not None else None, b.pooled, a, b.ctrl_x, b.ctrl_h, fused,
                         n_c1, n_c2, n_sc, n_c2t, n_c1t, n_sct, n_dimg))
    uses.append((tail[1], tail[0]))
    n = len(out)
    cut = max(1, n // 2) if n > 1 and not one_bucket else 0
    return DisPlan(tuple(out), tuple(tail), tuple(buffers), tuple(fwd), tuple(bwd), tuple(dimg), image_cin, tuple(uses), cut)
