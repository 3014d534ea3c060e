"""MCGatedPixelCNN.sample (pixelcnn_sampler.py, csrc/pixelcnn_sample.hip): incremental eval-mode ancestral sampling.
The logits at (i, j) of one full eval forward depend only on codes before (i, j), so ONE forward on the returned map
re-derives every position's logits and every draw: parity of the sampler's own logits, the inverse-CDF rule against
fp64, greedy decoding against the CPU oracle, and the contract shared with `generate`."""
import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _small(dtype=torch.float32):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    d = gu.load_npz('mcpixelcnn_small.npz')
    cfg.update(model_name='mcpixelcnn', device='cuda', classes_size=10, controller_rate=0.5, compute_dtype='float32')
    cfg['pixelcnn'] = {'num_layer': 4, 'hidden_size': 16, 'num_embedding': 32}
    m = models.mcpixelcnn()
    m.load_state_dict(gu.state_from_npz(d, 'sd_final/'))
    return m.cuda().train(False).set_compute_dtype(dtype)


def _perturb_bn(m, seed):
    g = torch.Generator().manual_seed(seed)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            c = mod.num_features
            mod.running_mean.copy_((torch.randn(c, generator=g) * 0.1).to(mod.running_mean.device))
            mod.running_var.copy_((torch.rand(c, generator=g) + 0.5).to(mod.running_var.device))
            mod.weight.data.copy_((torch.rand(c, generator=g) + 0.5).to(mod.weight.device))
            mod.bias.data.copy_((torch.randn(c, generator=g) * 0.1).to(mod.bias.device))
    return m


def _full(dtype=torch.float32):
    """configs[4]: hidden 128, 15 layers, 512 codes, 10 modes, seeded weights and perturbed BatchNorm statistics."""
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name='mcpixelcnn', device='cuda', classes_size=10, controller_rate=0.5, compute_dtype='float32')
    cfg['pixelcnn'] = {'num_layer': 15, 'hidden_size': 128, 'num_embedding': 512}
    torch.manual_seed(4)
    m = models.mcpixelcnn()
    return _perturb_bn(m, 5).cuda().train(False).set_compute_dtype(dtype)


def _forward_logits(m, codes, lab, dtype):
    m.set_compute_dtype(dtype)
    with torch.no_grad():
        return m({'img': codes, 'label': lab})['logits']


def _pow2(v):
    return v & (v - 1) == 0


def _reference_logits(m, codes, lab):
    """The engine's eval forward, or, where the engine does not run (H, W not powers of two), the CPU restatement of the
    schedule that test_pixelcnn_sample_cpu.py pins to the oracle (the oracle's crop is defined for square maps only)."""
    if _pow2(codes.shape[1]) and _pow2(codes.shape[2]):
        return _forward_logits(m, codes, lab, torch.float32)
    from test_pixelcnn_sample_cpu import schedule_forward
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    return schedule_forward(sd, codes.cpu(), lab.cpu(), m.output_conv[3].codebook.shape[0])


def _labels(n, seed=1):
    return torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(seed)).cuda()


def _check_parity(m, n, h, w, seed):
    lab = _labels(n, seed)
    torch.manual_seed(seed)
    x = torch.zeros((n, h, w), dtype=torch.long, device='cuda')
    m.set_compute_dtype(torch.float32)
    out, lg = m.sample(lab, x=x, return_logits=True)
    assert out is x and lg.shape == (n, m.input_size, h, w) and lg.dtype == torch.float32
    assert int(out.min()) >= 0 and int(out.max()) < m.input_size
    err = _rel(lg, _reference_logits(m, out, lab))
    assert err <= 1e-5, err
    xb = torch.zeros((n, h, w), dtype=torch.long, device='cuda')
    m.set_compute_dtype(torch.bfloat16)
    outb, lgb = m.sample(lab, x=xb, return_logits=True)
    e32 = _rel(lgb, _reference_logits(m, outb, lab))
    e16 = _rel(lgb, _forward_logits(m, outb, lab, torch.bfloat16)) if _pow2(h) and _pow2(w) else 0.0
    assert e16 <= 2e-2 and e32 <= 5e-2, (e16, e32)
    m.set_compute_dtype(torch.float32)
    return out, lg


@pytest.mark.parametrize('n,h,w', [(6, 8, 8), (37, 8, 8), (37, 5, 7), (1000, 8, 8)])
def test_sample_logit_parity_small(n, h, w):
    _check_parity(_perturb_bn(_small(), 11), n, h, w, seed=n + h)


@pytest.mark.parametrize('n,h,w', [(37, 8, 8), (6, 5, 7), (1000, 8, 8)])
def test_sample_logit_parity_full_width(n, h, w):
    _check_parity(_full(), n, h, w, seed=n + w)


def _inverse_cdf(lg, u):
    """fp64 inverse CDF of logits [N, K, H, W] at u [N, H, W] -> (codes, near a boundary)."""
    x = lg.double().permute(0, 2, 3, 1)
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    cs = e.cumsum(-1)
    s = cs[..., -1:]
    t = u.double().unsqueeze(-1) * s
    k = (cs <= t).sum(-1)
    near = ((cs - t).abs() < 1e-6 * s).any(-1)
    return k, near


@pytest.mark.parametrize('full', [False, True])
def test_sample_draw_rule_and_greedy(full):
    m = _full() if full else _perturb_bn(_small(), 3)
    n, h, w = 64, 8, 8
    lab = _labels(n, 2)
    u = torch.rand((h * w, n), generator=torch.Generator().manual_seed(6)).cuda()
    x, lg = m.sample(lab, uniform=u, return_logits=True)
    k, near = _inverse_cdf(lg.cpu(), u.t().reshape(n, h, w).cpu())
    ok = (k == x.cpu()) | near
    assert bool(ok.all()), f'{int((~ok).sum())} draws differ from the fp64 inverse CDF'
    assert float(near.float().mean()) < 0.01
    g, lgg = m.sample(lab, greedy=True, return_logits=True)
    top = lgg.cpu().topk(2, dim=1)
    agree = top.indices[:, 0] == g.cpu()
    tie = (top.values[:, 0] - top.values[:, 1]) < 1e-4
    assert bool((agree | tie).all())


def test_sample_greedy_vs_oracle():
    """As test_generate_autoregressive_greedy_vs_oracle: one CPU oracle forward on the greedy map re-derives every
    decision (argmax, or a top-2 tie below 1e-4)."""
    from oracle import mcpixelcnn_oracle as O
    d = gu.load_npz('mcpixelcnn_small.npz')
    sd = gu.state_from_npz(d, 'sd_final/')
    m = _small()
    lab = torch.from_numpy(d['label']).cuda()
    codes = m.sample(lab, greedy=True)
    assert codes.shape == (6, 8, 8) and codes.dtype == torch.int64
    ref = O.forward({k: v.clone() for k, v in sd.items()}, codes.cpu(), lab.cpu(), 10, train=False)['logits']
    top = ref.topk(2, dim=1)
    agree = top.indices[:, 0] == codes.cpu()
    tie = (top.values[:, 0] - top.values[:, 1]) < 1e-4
    assert bool((agree | tie).all()), f'{int((~(agree | tie)).sum())} of 384 greedy decisions differ from the oracle'
    assert float(agree.float().mean()) > 0.98


def test_sample_contract():
    m = _perturb_bn(_small(), 4)
    n = 37
    lab = _labels(n, 8)
    u = torch.rand((64, n), generator=torch.Generator().manual_seed(1)).cuda()
    x = torch.zeros((n, 8, 8), dtype=torch.long, device='cuda')
    out = m.sample(lab, x=x, uniform=u)
    assert out is x                                                     # written in place and returned
    junk = torch.randint(-5, 1000, (n, 8, 8), generator=torch.Generator().manual_seed(9)).cuda()
    assert torch.equal(m.sample(lab, x=junk, uniform=u), out)           # prior contents are never read
    torch.manual_seed(3)
    a = m.sample(lab)
    torch.manual_seed(3)
    b = m.sample(lab)
    assert torch.equal(a, b) and a.shape == (n, 8, 8) and int(a.min()) >= 0 and int(a.max()) < 32
    m.train(True)
    with pytest.raises(ValueError, match='Not valid'):
        m.sample(lab)
    m.train(False)
    with pytest.raises(ValueError, match='Not valid'):
        m.sample(torch.full((n,), 10, dtype=torch.long, device='cuda'))
    with pytest.raises(ValueError, match='Not valid'):
        m.sample(lab.int())


def test_sample_after_create_follows_new_codebooks():
    from mcgen_amd.config import cfg
    from mcgen_amd.models import utils as mutils
    m = _perturb_bn(_small(), 12)
    cfg['classes_size'] = 4
    torch.manual_seed(0)
    mutils.create(m)
    assert m.output_conv[3].codebook.shape[0] == 4
    lab = _labels(20, 4) % 4
    x, lg = m.sample(lab, return_logits=True)
    assert _rel(lg, _forward_logits(m, x, lab, torch.float32)) <= 1e-5
    with pytest.raises(ValueError, match='Not valid'):
        m.sample(torch.full((3,), 5, dtype=torch.long, device='cuda'))
    cfg['classes_size'] = 10


# ---- driver: train_vqvae -> train_pixelcnn -> generate ------------------------------------------------------------------
def _run(args, cwd):
    import os
    import subprocess
    import sys
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_generate_driver_after_training(tmp_path):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    drv = os.path.join(root, 'compat')
    common = ['--data_name', 'CIFAR10', '--log_interval', '0.5']
    _run([os.path.join(drv, 'train_vqvae.py'), '--model_name', 'vqvae', '--control_name', 'None', '--num_epochs', '1',
          '--synthetic_size', '200', '--batch', '64'] + common, tmp_path)
    _run([os.path.join(drv, 'train_pixelcnn.py'), '--model_name', 'mcpixelcnn', '--control_name', '0.5', '--num_epochs', '1',
          '--synthetic_size', '192', '--batch', '64'] + common, tmp_path)
    tag = '0_CIFAR10_label_mcpixelcnn_0.5'
    assert (tmp_path / 'output' / 'model' / f'{tag}_best.pt').exists()
    gen = [os.path.join(drv, 'generate.py'), '--model_name', 'mcpixelcnn', '--control_name', '0.5', '--save_npy', 'True',
           '--generate_per_mode', '3', '--synthetic_size', '192'] + common
    out = _run(gen, tmp_path)
    assert f'Experiment: {tag}' in out and 'Not exists model tag' not in out
    npy = tmp_path / 'output' / 'npy' / f'generated_{tag}.npy'
    a = np.load(npy)
    assert a.shape == (30, 3, 32, 32) and np.isfinite(a).all() and a.min() >= 0 and a.max() <= 255
    assert (tmp_path / 'output' / 'vis' / f'generated_{tag}.npy').exists()            # the image grid (save_img)
    os.remove(npy)
    _run(gen, tmp_path)
    assert np.array_equal(np.load(npy), a)                                             # seeded: identical across runs
    # the grid branch (save_npy False): 10 modes x save_per_mode
    _run([os.path.join(drv, 'generate.py'), '--model_name', 'mcpixelcnn', '--control_name', '0.5', '--save_per_mode', '2',
          '--synthetic_size', '192'] + common, tmp_path)
    grid = np.load(tmp_path / 'output' / 'vis' / f'generated_{tag}_10.npy')
    assert grid.shape == (20, 3, 32, 32) and np.isfinite(grid).all()
