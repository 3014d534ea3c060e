"""CPU-side checks of MCGatedPixelCNN.sample (no GPU): argument validation raises before any launch, and a torch
restatement of the row / column schedule that csrc/pixelcnn_sample.hip implements (every pixel of every layer computed
once: row phase = vertical stacks, gate_v, vert_to_horiz of one row; column phase = horizontal path and head of one
position) reproduces the oracle's full eval forward."""
import ctypes

import pytest
import torch
import torch.nn.functional as F


def _model(hidden=16, layers=4, codes=32, modes=10):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name='mcpixelcnn', device='cpu', classes_size=modes, controller_rate=0.5, compute_dtype='float32')
    cfg['pixelcnn'] = {'num_layer': layers, 'hidden_size': hidden, 'num_embedding': codes}
    torch.manual_seed(0)
    return models.mcpixelcnn()


def test_sample_validates_before_any_launch():
    m = _model()
    lab = torch.arange(4) % 10
    m.train(True)
    with pytest.raises(ValueError, match='Not valid'):
        m.sample(lab)                                                   # batch-statistics BatchNorm: not incremental
    m.train(False)
    with pytest.raises(ValueError, match='Not valid'):
        m.sample(lab.int())
    with pytest.raises(ValueError, match='Not valid'):
        m.sample(torch.tensor([0, 10]))
    with pytest.raises(ValueError, match='Not valid'):
        m.sample(torch.tensor([-1, 3]))


def test_library_exports_sampler_symbols():
    from mcgen_amd import _lib
    if not __import__('os').path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mcgen_px_sample_row', 'mcgen_px_sample_col', 'mcgen_px_sample_weight_elems'):
        assert hasattr(raw, name) and name in _lib.SYMBOLS, name
    # host-side checks reject a null descriptor before any launch
    P = _lib.PxSample()
    assert lib.mcgen_px_sample_row(ctypes.byref(P), 0, 0, None) != 0
    assert b'px_sample' in lib.mcgen_last_error()
    # the weight pack holds every stack / link / head weight once (plus the zero padding of the MFMA tiles)
    m = _model(hidden=128, layers=15, codes=512)
    live = sum(p.numel() for n, p in m.named_parameters() if n.endswith('weight') and p.dim() == 4)
    live -= m.layers[0].vert_stack.weight[:, :, -1].numel() + m.layers[0].horiz_stack.weight[..., -1].numel()
    assert lib.mcgen_px_sample_weight_elems(128, 15, 512, 512) == live


def _affine(sd, p):
    sc = sd[p + 'weight'] / torch.sqrt(sd[p + 'running_var'] + 1e-5)
    return sc, sd[p + 'bias'] - sd[p + 'running_mean'] * sc


def _gate(x, sd, p, code):
    a, b = x.chunk(2, dim=-1)
    sc, sh = _affine(sd, p + 'bn.')
    return code * torch.relu(a * sc + sh) * torch.sigmoid(b)


def schedule_forward(sd, codes, label, classes):
    """The sampler's decomposition in torch, teacher-forced on `codes` [N, H, W]: H row phases and H*W column phases,
    every pixel of every layer computed once, caches of one row (out_v: two rows) -> logits [N, K, H, W].  Indexing is
    per coordinate, so a non-square map is causal too (the reference crops the horizontal stack to H columns, mcpixelcnn.py:53,
    which is defined only for square maps)."""
    n, h, w = codes.shape
    n_layer = 1 + max(int(k.split('.')[1]) for k in sd if k.startswith('layers.'))
    ind = F.one_hot(label, classes).float()
    mc = lambda name: ind @ sd[name + '.codebook']                                      # noqa: E731
    emb = F.embedding(codes, sd['embedding.weight'])                                  # [N, H, W, C]
    c = emb.shape[-1]
    wv0 = sd['layers.0.vert_stack.weight'][:, :, :3]                                  # live taps of the mask-A stacks
    wh0 = sd['layers.0.horiz_stack.weight'][..., :3]
    out_v = [torch.zeros(n, 2, w, c) for _ in range(n_layer)]                        # ring of rows i-1, i per layer
    v2h = [None] * n_layer
    xh = [torch.zeros(n, w, c) for _ in range(n_layer)]                              # x_h of the current row per layer
    logits = torch.zeros(n, sd['output_conv.4.module.weight'].shape[0], h, w)
    for i in range(h):
        # ---- row phase: vertical stacks, gate_v and vert_to_horiz of row i
        for l in range(n_layer):
            p = f'layers.{l}.'
            hv = sd[p + 'vert_stack.bias'].expand(n, w, 2 * c).clone()
            for j in range(w):
                if l == 0:
                    taps = [(i - 3 + dr, j - 3 + dc, wv0[:, :, dr, dc]) for dr in range(3) for dc in range(7)]
                    src = lambda r, col: emb[:, r, col]                              # noqa: E731
                else:
                    wv = sd[p + 'vert_stack.weight']
                    taps = [(i - 1 + dr, j - 1 + dc, wv[:, :, dr, dc]) for dr in range(2) for dc in range(3)]
                    src = lambda r, col, l=l: out_v[l - 1][:, (r - i) + 1, col]      # noqa: E731
                for r, col, wt in taps:
                    if 0 <= r and 0 <= col < w:
                        hv[:, j] += src(r, col) @ wt.t()
            v2h[l] = hv @ sd[p + 'vert_to_horiz.weight'][:, :, 0, 0].t() + sd[p + 'vert_to_horiz.bias']
            new = _gate(hv, sd, p + 'gate_v.', mc(p + 'gate_v.mc')[:, None])
            out_v[l] = torch.stack([out_v[l][:, 1], new], 1)                       # rows i-1, i
        # ---- column phases: horizontal path, head of (i, j)
        for j in range(w):
            x_prev = None
            for l in range(n_layer):
                p = f'layers.{l}.'
                s = sd[p + 'horiz_stack.bias'] + v2h[l][:, j]
                if l == 0:
                    for dc in range(3):
                        if j - 3 + dc >= 0:
                            s = s + emb[:, i, j - 3 + dc] @ wh0[:, :, 0, dc].t()
                else:
                    wh = sd[p + 'horiz_stack.weight']
                    if j > 0:
                        s = s + xh[l - 1][:, j - 1] @ wh[:, :, 0, 0].t()
                    s = s + x_prev @ wh[:, :, 0, 1].t()
                oh = _gate(s, sd, p + 'gate_h.', mc(p + 'gate_h.mc'))
                r = oh @ sd[p + 'horiz_resid.0.module.weight'][:, :, 0, 0].t() + sd[p + 'horiz_resid.0.module.bias']
                sc, sh = _affine(sd, p + 'horiz_resid.1.module.')
                x = (r * sc + sh) * mc(p + 'horiz_resid.2')
                if l > 0:
                    x = x + x_prev
                xh[l][:, j] = x
                x_prev = x
            h0 = x_prev @ sd['output_conv.0.module.weight'][:, :, 0, 0].t() + sd['output_conv.0.module.bias']
            sc, sh = _affine(sd, 'output_conv.1.module.')
            z = torch.relu(h0 * sc + sh) * mc('output_conv.3')
            logits[:, :, i, j] = z @ sd['output_conv.4.module.weight'][:, :, 0, 0].t() + sd['output_conv.4.module.bias']
    return logits


@pytest.mark.parametrize('h,w', [(8, 8), (5, 5)])
def test_row_column_schedule_matches_oracle(h, w):
    from oracle import mcpixelcnn_oracle as O
    m = _model(hidden=16, layers=4, codes=32)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, t in m.state_dict().items():
            if t.is_floating_point() and 'codebook' not in name:
                t.copy_(torch.randn(t.shape, generator=g) * 0.3)
            if 'running_var' in name:
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    m.layers[0].make_causal()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    codes = torch.randint(0, 32, (5, h, w), generator=g)
    label = torch.randint(0, 10, (5,), generator=g)
    ref = O.forward({k: v.clone() for k, v in sd.items()}, codes, label, 10, train=False)['logits']
    got = schedule_forward(sd, codes, label, 10)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-5
