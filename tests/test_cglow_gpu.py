"""GPU parity of the CGlow label-conditioned prior kernels against their float64 restatement (tests/cglow_ref.py) and of the
CGlow likelihood forward / backward / training step / reverse / generate on the HIP path against the reference-generated
fixtures (tests/golden/cglow_*.npz).  Kernel tolerances: test_cvae_gpu.py's for its label kernels (5e-5 fp32, 1e-2 bf16, of
the tensor's max); model tolerances: test_mcglow_gpu.py's for the same quantities."""
import numpy as np
import pytest
import torch

import cglow_ref as R

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _model(sd, classes, channels, dtype=torch.float32):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name='cglow', device='cuda', classes_size=classes, data_shape=[channels, 32, 32], compute_dtype='float32')
    cfg['glow'] = dict(R.GLOW_CFG)
    np.random.seed(0)
    m = models.cglow()
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    return m.set_compute_dtype(dtype) if dtype != torch.float32 else m


def _batch(d):
    return torch.from_numpy(d['img']).cuda(), torch.from_numpy(d['label']).cuda()


def _noise(d, tag):
    return torch.from_numpy(d[f'noise/{tag}/0']).cuda()


# ---- kernels ------------------------------------------------------------------------------------------------------------------
def _kernel_case(modes, c2, hw, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    n = 9
    p = {k: 0.3 * torch.randn(c2, generator=g) for k in ('b_p', 's_p', 'b_e', 's_e')}
    p['w_e'] = 0.3 * torch.randn(c2, modes, 1, 1, generator=g)
    label = torch.randint(0, modes, (n,), generator=g)
    label[0] = modes - 1; label[1] = label[2]; label[5] = 0                # the last mode, a repeat, the first mode
    cp = (c2 + 7) // 8 * 8
    side = int(hw ** 0.5)
    dprior = torch.randn(n, side, side, cp, generator=g).to(dtype)         # the pad channels hold values too: they must be ignored
    return p, label, dprior, cp, side


def _args(p, dev='cuda'):
    return [p[k].to(dev) for k in ('b_p', 's_p', 'w_e', 'b_e', 's_e')]


def _np_args(p):
    c2 = p['b_p'].numel()
    return [p['b_p'].numpy(), p['s_p'].numpy(), p['w_e'].reshape(c2, -1).numpy(), p['b_e'].numpy(), p['s_e'].numpy()]


def _run_bwd(ops, p, label, dprior, c):
    c2, modes = p['w_e'].shape[:2]
    out = {k: torch.full((c2,), float('nan'), device='cuda') for k in ('b_p', 's_p', 'b_e', 's_e')}
    out['w_e'] = torch.full((c2, modes, 1, 1), float('nan'), device='cuda')
    out['w_p'] = torch.full((c2, c, 3, 3), float('nan'), device='cuda')
    ops.cglow_prior_bwd(dprior.cuda(), *_args(p), label.cuda(), out['b_p'], out['s_p'], out['w_p'], out['w_e'], out['b_e'], out['s_e'])
    return out


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('hw', [16, 4])
@pytest.mark.parametrize('modes,c2', [(10, 96), (1623, 32), (12, 8), (40, 12)])         # (40, 12): a padded row, Cp = 16
def test_prior_kernels_vs_float64(modes, c2, hw, dtype):
    from mcgen_amd import ops
    f32 = dtype == torch.float32
    tol = 5e-5 if f32 else 1e-2
    p, label, dprior, cp, side = _kernel_case(modes, c2, hw, dtype, 1000 * modes + c2 + hw)
    n, c = label.numel(), c2 // 2
    # forward
    out = ops.cglow_prior(*_args(p), label.cuda(), side, side, dtype)
    assert out.shape == (n, side, side, cp) and out.dtype == dtype
    ref = R.prior(*_np_args(p), label.numpy(), hw).reshape(n, side, side, c2)
    print('prior rel err', _rel(out[..., :c2].float(), ref))
    assert _rel(out[..., :c2].float(), ref) < tol
    if cp > c2:
        assert float(out[..., c2:].float().abs().max()) == 0.0
    assert torch.equal(out, out[:, :1, :1, :].expand_as(out))                            # the same at every pixel
    assert torch.equal(out, ops.cglow_prior(*_args(p), label.cuda(), side, side, dtype))
    # backward, from the gradient as the kernel reads it (rounded to the compute dtype)
    gref = R.prior_bwd(dprior[..., :c2].double().reshape(n, hw, c2).numpy(), *_np_args(p), label.numpy())
    got = _run_bwd(ops, p, label, dprior, c)
    for k, v in gref.items():
        err = _rel(got[k].reshape(v.shape), v)
        print('prior_bwd rel err', k, err)
        assert err < tol, k
    assert float(got['w_p'].abs().max()) == 0.0                                          # prior.conv.weight reads only zeros
    absent = torch.ones(modes, dtype=torch.bool); absent[label] = False
    assert float(got['w_e'][:, absent.cuda()].abs().max()) == 0.0
    again = _run_bwd(ops, p, label, dprior, c)
    assert all(torch.equal(got[k], again[k]) for k in got)
    # labels outside the table: a zero embedding row forward, skipped in the table gradient, nothing read outside the table
    bad = label.clone(); bad[3] = modes; bad[4] = -1; bad[6] = 2 ** 40
    outb = ops.cglow_prior(*_args(p), bad.cuda(), side, side, dtype)
    refb = R.prior(*_np_args(p), bad.numpy(), hw).reshape(n, side, side, c2)
    assert _rel(outb[..., :c2].float(), refb) < tol
    gotb = _run_bwd(ops, p, bad, dprior, c)
    grefb = R.prior_bwd(dprior[..., :c2].double().reshape(n, hw, c2).numpy(), *_np_args(p), bad.numpy())
    for k, v in grefb.items():
        assert _rel(gotb[k].reshape(v.shape), v) < tol, k
    absent = torch.ones(modes, dtype=torch.bool); absent[bad[(bad >= 0) & (bad < modes)]] = False
    assert float(gotb['w_e'][:, absent.cuda()].abs().max()) == 0.0


def test_prior_wrappers_refuse_bad_tensors():
    from mcgen_amd import _lib, ops
    p, label, dprior, cp, side = _kernel_case(12, 8, 4, torch.float32, 5)
    a = _args(p)
    with pytest.raises(_lib.McgenError):
        ops.cglow_prior(*_args(p, 'cpu'), label, side, side, torch.float32)                                 # no CPU path
    with pytest.raises(_lib.McgenError):
        ops.cglow_prior(*a, label.int().cuda(), side, side, torch.float32)                                  # int64 labels only
    with pytest.raises(_lib.McgenError):
        ops.cglow_prior(a[0], a[1][:4], a[2], a[3], a[4], label.cuda(), side, side, torch.float32)          # a short scale
    with pytest.raises(_lib.McgenError):
        ops.cglow_prior(*a, label.cuda(), side, side, torch.float16)                                        # no such compute dtype
    g = [torch.zeros(8, device='cuda') for _ in range(4)]
    with pytest.raises(_lib.McgenError):                                                                    # one label short
        ops.cglow_prior_bwd(dprior.cuda(), *a, label[:-1].cuda(), g[0], g[1], None, torch.zeros(8, 12, device='cuda'), g[2], g[3])
    with pytest.raises(_lib.McgenError):                                                                    # a table gradient of another size
        ops.cglow_prior_bwd(dprior.cuda(), *a, label.cuda(), g[0], g[1], None, torch.zeros(8, 11, device='cuda'), g[2], g[3])


# ---- model against the fixtures ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fixture,classes,channels', R.FIXTURES)
def test_cglow_forward_init_and_reverse(fixture, classes, channels):
    d = R.load(fixture)
    sd0, init, final = R.states(d)
    img, lab = _batch(d)
    # 1. data-dependent ActNorm initialisation on the first training forward (train_glow.py:60-67)
    m = _model(sd0, classes, channels)
    m.train(True)
    with torch.no_grad():
        m({'img': img, 'label': lab, 'noise': _noise(d, 'init')})
    sd = m.state_dict()
    for k, v in init.items():
        if k.endswith(('loc', 'scale')):
            assert float((sd[k].cpu() - v).abs().max()) < 2e-3 * float(v.abs().max()) + 1e-5, k
        if k.endswith('initialized'):
            assert int(sd[k]) == 1
    # 2. training-mode likelihood on the initialised weights = first logged loss of the fixture
    m = _model(init, classes, channels)
    m.train(True)
    out = m({'img': img, 'label': lab, 'noise': _noise(d, 0)})
    print('loss', float(out['loss'].detach()), float(d['losses'][0]))
    assert abs(float(out['loss'].detach()) - float(d['losses'][0])) < 1e-4
    for i, z in enumerate(out['z']):
        assert _rel(z, d[f'z0/{i}']) < 5e-4, i
    # 3. eval forward, reverse(reconstruct) and generate on the reference's final weights
    m = _model(final, classes, channels)
    m.train(False)
    out = m({'img': img, 'label': lab, 'noise': _noise(d, 'eval')})
    assert abs(float(out['loss']) - float(d['loss_eval'])) < 1e-4
    rec = m.reverse({'z': out['z'], 'label': lab, 'reconstruct': True})['img']
    assert _rel(rec, d['reconstructed']) < 1e-3
    gz = [torch.from_numpy(d[f'gen_z/{i}']).cuda() for i in range(3)]
    gen = m.generate(lab, gz)
    assert _rel(gen, d['generated']) < 1e-3
    assert gen.shape == img.shape and bool(torch.isfinite(gen).all()) and float(gen.abs().max()) <= 1.0
    # the label reaches the samples: another label, another image
    other = (lab + 1) % classes
    assert float((m.generate(other, gz) - gen).abs().max()) > 1e-4
    # generate with drawn latents
    free = m.generate(lab)
    assert free.shape == img.shape and bool(torch.isfinite(free).all()) and float(free.abs().max()) <= 1.0


@pytest.mark.parametrize('fixture,classes,channels', R.FIXTURES)
def test_cglow_gradients_vs_reference(fixture, classes, channels):
    """d(bits/dim)/d(every parameter) of the first training step, through loss.backward(), against the reference's autograd."""
    d = R.load(fixture)
    _, init, _ = R.states(d)
    img, lab = _batch(d)
    m = _model(init, classes, channels)
    m.train(True)
    out = m({'img': img, 'label': lab, 'noise': _noise(d, 0)})
    out['loss'].backward()
    named = dict(m.named_parameters())
    gref = {k[len('grad0/'):]: torch.from_numpy(v) for k, v in d.items() if k.startswith('grad0/')}
    unused = {f'blocks.{i}.embedding.{leaf}' for i in range(2) for leaf in ('scale', 'conv.weight', 'conv.bias')}
    assert set(named) == set(gref) | unused and not set(gref) & unused
    worst = 0.0
    for k, gr in gref.items():
        gg = named[k].grad
        assert gg is not None, k
        err = float((gg.cpu() - gr).abs().max())
        tol = 2e-4 * float(gr.abs().max()) + 1e-6
        assert err < tol, (k, err, tol)
        worst = max(worst, err / tol)
    print('worst err/tol', worst)
    for k in unused:                                                                     # as in the reference: no gradient at all
        assert named[k].grad is None, k
    assert float(named['blocks.2.prior.conv.weight'].grad.abs().max()) == 0.0
    absent = torch.ones(classes, dtype=torch.bool); absent[lab.cpu()] = False
    assert float(named['blocks.2.embedding.conv.weight'].grad[:, absent.cuda()].abs().max()) == 0.0


def _check_final(m, d, final, init):
    sd = m.state_dict()
    far = 0
    for k, v in final.items():
        if not v.dtype.is_floating_point:
            continue
        diff = (sd[k].cpu() - v).abs()
        assert float(diff.max()) < 1.3e-3, (k, float(diff.max()))
        far += int((diff > 1e-5 + 1e-3 * v.abs()).sum())
    total = sum(v.numel() for v in final.values() if v.dtype.is_floating_point)
    assert far < 0.02 * total, (far, total)
    for i in range(2):                                   # Adam sees zero gradients with zero moments: bit-unchanged
        for leaf in ('scale', 'conv.weight', 'conv.bias'):
            k = f'blocks.{i}.embedding.{leaf}'
            assert torch.equal(sd[k].cpu(), init[k]), k
    assert torch.equal(sd['blocks.2.prior.conv.weight'].cpu(), init['blocks.2.prior.conv.weight'])


def _loss_bounds(n):
    return [1e-4, 5e-4][:n]


@pytest.mark.parametrize('fixture,classes,channels', R.FIXTURES)
def test_cglow_training_steps_vs_reference(fixture, classes, channels):
    """train_glow.py loop body (clip_grad_norm_ 1, Adam 3e-4) from the fixture's initialised weights: logged losses and final
    weights, test_mcglow_gpu.py's bounds (Adam's first steps move a weight whose gradient is rounding noise by up to
    2 * lr per step)."""
    from mcgen_amd.trainer import GlowTrainer
    d = R.load(fixture)
    _, init, final = R.states(d)
    img, lab = _batch(d)
    m = _model(init, classes, channels)
    tr = GlowTrainer(m)
    steps = len(d['losses'])
    losses = [float(tr.train_iteration(img, lab, _noise(d, s))) for s in range(steps)]
    print('losses', losses, 'reference', d['losses'])
    for got, ref, tol in zip(losses, d['losses'], _loss_bounds(steps)):
        assert abs(got - ref) < tol, (losses, d['losses'])
    _check_final(m, d, final, init)


@pytest.mark.parametrize('fixture,classes,channels', R.FIXTURES)
def test_cglow_graphed_trainer_tracks_eager(fixture, classes, channels):
    """HIP-graph replay of the train step: capture leaves the weights untouched, and replays with the fixture's
    dequantisation noise injected reproduce the reference's logged losses and the eager trainer's."""
    from mcgen_amd.trainer import GlowTrainer
    d = R.load(fixture)
    _, init, final = R.states(d)
    img, lab = _batch(d)
    ma, mb = _model(init, classes, channels), _model(init, classes, channels)
    ta, tb = GlowTrainer(ma), GlowTrainer(mb)
    tb.capture(img, lab, warmup=1)
    for k, v in mb.state_dict().items():
        assert torch.equal(v.cpu(), init[k]), k
    steps = len(d['losses'])
    la = [float(ta.train_iteration(img, lab, _noise(d, s))) for s in range(steps)]
    lb = [float(tb.train_iteration(img, lab, _noise(d, s))) for s in range(steps)]
    for got, ref, tol in zip(lb, d['losses'], _loss_bounds(steps)):
        assert abs(got - ref) < tol, (lb, d['losses'])
    assert max(abs(x - y) for x, y in zip(la, lb)) < 1e-5, (la, lb)
    _check_final(mb, d, final, init)
    lc = [float(tb.train_iteration(img, lab)) for _ in range(2)]           # without injected noise the graph draws its own
    assert all(np.isfinite(lc))


@pytest.mark.parametrize('fixture,classes,channels', R.FIXTURES)
def test_cglow_bf16_tracks_fp32(fixture, classes, channels):
    """bf16 compute (fp32 accumulation, fp32 log-determinants): test_mcglow_gpu.py's bf16 bounds on the likelihood and on
    the training steps' losses."""
    from mcgen_amd.trainer import GlowTrainer
    d = R.load(fixture)
    _, init, _ = R.states(d)
    img, lab = _batch(d)
    m = _model(init, classes, channels, torch.bfloat16)
    m.train(True)
    with torch.no_grad():
        out = m({'img': img, 'label': lab, 'noise': _noise(d, 0)})
    print('bf16 loss', float(out['loss']), float(d['losses'][0]))
    assert abs(float(out['loss']) - float(d['losses'][0])) < 2e-2
    tr = GlowTrainer(m)
    steps = len(d['losses'])
    losses = [float(tr.train_iteration(img, lab, _noise(d, s))) for s in range(steps)]
    print('bf16 losses', losses, d['losses'])
    for got, ref, tol in zip(losses, d['losses'], [2e-2, 3e-2]):
        assert abs(got - ref) < tol, (losses, d['losses'])
    sd = m.state_dict()
    for i in range(2):
        for leaf in ('scale', 'conv.weight', 'conv.bias'):
            k = f'blocks.{i}.embedding.{leaf}'
            assert torch.equal(sd[k].cpu(), init[k]), k
    m.train(False)
    gen = m.generate(lab)
    assert bool(torch.isfinite(gen).all()) and float(gen.abs().max()) <= 1.0
