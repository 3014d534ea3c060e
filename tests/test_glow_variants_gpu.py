"""GPU parity of MCGlow with additive coupling and / or the plain InvConv2d (cfg glow.affine / glow.conv_lu = False) on the HIP
path against the reference-generated fixtures tests/golden/mcglow_{additive,plainconv,plain_additive_cifar}_small.npz:
likelihood forward with the ActNorm initialisation, backward, training steps (eager and graphed), reverse, generate, bf16,
and the create surgery.  The tests and every bound are test_cglow_gpu.py's, which takes them from test_mcglow_gpu.py for
the same quantities."""
import numpy as np
import pytest
import torch

import glow_variants_ref as R

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _model(sd, classes, channels, affine, conv_lu, dtype=torch.float32):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name='mcglow', device='cuda', classes_size=classes, data_shape=[channels, 32, 32], compute_dtype='float32',
               controller_rate=0.5)
    cfg['glow'] = R.glow_cfg(affine, conv_lu)
    np.random.seed(0)
    m = models.mcglow()
    m.load_state_dict(sd, strict=True)
    m = m.cuda()
    return m.set_compute_dtype(dtype) if dtype != torch.float32 else m


def _batch(d):
    return torch.from_numpy(d['img']).cuda(), torch.from_numpy(d['label']).cuda()


def _noise(d, tag):
    return torch.from_numpy(d[f'noise/{tag}/0']).cuda()


@pytest.mark.parametrize('fixture,classes,channels,affine,conv_lu', R.FIXTURES)
def test_forward_init_and_reverse(fixture, classes, channels, affine, conv_lu):
    d = R.load(fixture)
    sd0, init, final = R.states(d)
    img, lab = _batch(d)
    # 1. data-dependent ActNorm initialisation on the first training forward (train_glow.py:60-67)
    m = _model(sd0, classes, channels, affine, conv_lu)
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
    m = _model(init, classes, channels, affine, conv_lu)
    m.train(True)
    out = m({'img': img, 'label': lab, 'noise': _noise(d, 0)})
    print('loss', float(out['loss'].detach()), float(d['losses'][0]))
    assert abs(float(out['loss'].detach()) - float(d['losses'][0])) < 1e-4
    for i, z in enumerate(out['z']):
        assert _rel(z, d[f'z0/{i}']) < 5e-4, i
    # 3. eval forward, reverse(reconstruct) and generate on the reference's final weights
    m = _model(final, classes, channels, affine, conv_lu)
    m.train(False)
    out = m({'img': img, 'label': lab, 'noise': _noise(d, 'eval')})
    print('eval loss', float(out['loss']), float(d['loss_eval']))
    assert abs(float(out['loss']) - float(d['loss_eval'])) < 1e-4
    rec = m.reverse({'z': out['z'], 'label': lab, 'reconstruct': True})['img']
    assert _rel(rec, d['reconstructed']) < 1e-3
    gz = [torch.from_numpy(d[f'gen_z/{i}']).cuda() for i in range(3)]
    gen = m.generate(lab, gz)
    print('reverse / generate rel err', _rel(rec, d['reconstructed']), _rel(gen, d['generated']))
    assert _rel(gen, d['generated']) < 1e-3
    assert gen.shape == img.shape and bool(torch.isfinite(gen).all()) and float(gen.abs().max()) <= 1.0
    # the label reaches the samples: another label, another image
    other = (lab + 1) % classes
    assert float((m.generate(other, gz) - gen).abs().max()) > 1e-4
    free = m.generate(lab)
    assert free.shape == img.shape and bool(torch.isfinite(free).all()) and float(free.abs().max()) <= 1.0


@pytest.mark.parametrize('fixture,classes,channels,affine,conv_lu', R.FIXTURES)
def test_gradients_vs_reference(fixture, classes, channels, affine, conv_lu):
    """d(bits/dim)/d(every parameter) of the first training step, through loss.backward(), against the reference's autograd."""
    d = R.load(fixture)
    _, init, _ = R.states(d)
    img, lab = _batch(d)
    m = _model(init, classes, channels, affine, conv_lu)
    m.train(True)
    out = m({'img': img, 'label': lab, 'noise': _noise(d, 0)})
    out['loss'].backward()
    named = dict(m.named_parameters())
    gref = {k[len('grad0/'):]: torch.from_numpy(v) for k, v in d.items() if k.startswith('grad0/')}
    assert set(named) == set(gref)
    assert ('blocks.0.flows.0.invconv.weight' in named) == (not conv_lu)
    worst = 0.0
    for k, gr in gref.items():
        gg = named[k].grad
        assert gg is not None, k
        err = float((gg.cpu() - gr).abs().max())
        tol = 2e-4 * float(gr.abs().max()) + 1e-6
        assert err < tol, (k, err, tol)
        worst = max(worst, err / tol)
    print('worst err/tol', worst)
    assert float(named['blocks.2.prior.conv.weight'].grad.abs().max()) == 0.0          # the last prior reads only zeros
    if not conv_lu:
        # the weight's gradient is not the bare 1x1 weight gradient: the log-determinant adds -HW / (log 2 D) W^-T, which is
        # far outside the bound above in this fixture -- a kernel that dropped it could not pass
        npix = float(img[0].numel())
        for b, hw in enumerate((256, 64, 16)):
            k = f'blocks.{b}.flows.0.invconv.weight'
            w = init[k][:, :, 0, 0].double()
            term = -hw / (np.log(2.) * npix) * torch.linalg.inv(w).T
            assert float(term.abs().max()) > 100 * (2e-4 * float(gref[k].abs().max()) + 1e-6), k


def _check_final(m, final, init):
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
    # Adam sees a zero gradient with zero moments: bit-unchanged
    assert torch.equal(sd['blocks.2.prior.conv.weight'].cpu(), init['blocks.2.prior.conv.weight'])


@pytest.mark.parametrize('fixture,classes,channels,affine,conv_lu', R.FIXTURES)
def test_training_steps_vs_reference(fixture, classes, channels, affine, conv_lu):
    """train_glow.py loop body (clip_grad_norm_ 1, Adam 3e-4) from the fixture's initialised weights: logged losses and final
    weights, test_mcglow_gpu.py's bounds (Adam's first steps move a weight whose gradient is rounding noise by up to
    2 * lr per step)."""
    from mcgen_amd.trainer import GlowTrainer
    d = R.load(fixture)
    _, init, final = R.states(d)
    img, lab = _batch(d)
    m = _model(init, classes, channels, affine, conv_lu)
    tr = GlowTrainer(m)
    losses = [float(tr.train_iteration(img, lab, _noise(d, s))) for s in range(2)]
    print('losses', losses, 'reference', d['losses'])
    for got, ref, tol in zip(losses, d['losses'], [1e-4, 5e-4]):
        assert abs(got - ref) < tol, (losses, d['losses'])
    _check_final(m, final, init)
    if not conv_lu:                                      # the flat parameter buffer carries the plain weight: it moved
        k = 'blocks.1.flows.0.invconv.weight'
        assert not torch.equal(m.state_dict()[k].cpu(), init[k])


@pytest.mark.parametrize('fixture,classes,channels,affine,conv_lu', R.FIXTURES)
def test_graphed_trainer_tracks_eager(fixture, classes, channels, affine, conv_lu):
    """HIP-graph replay of the train step: capture leaves the weights untouched, and replays with the fixture's
    dequantisation noise injected reproduce the reference's logged losses and the eager trainer's."""
    from mcgen_amd.trainer import GlowTrainer
    d = R.load(fixture)
    _, init, final = R.states(d)
    img, lab = _batch(d)
    ma, mb = _model(init, classes, channels, affine, conv_lu), _model(init, classes, channels, affine, conv_lu)
    ta, tb = GlowTrainer(ma), GlowTrainer(mb)
    tb.capture(img, lab, warmup=1)
    for k, v in mb.state_dict().items():
        assert torch.equal(v.cpu(), init[k]), k
    la = [float(ta.train_iteration(img, lab, _noise(d, s))) for s in range(2)]
    lb = [float(tb.train_iteration(img, lab, _noise(d, s))) for s in range(2)]
    for got, ref, tol in zip(lb, d['losses'], [1e-4, 5e-4]):
        assert abs(got - ref) < tol, (lb, d['losses'])
    assert max(abs(x - y) for x, y in zip(la, lb)) < 1e-5, (la, lb)
    _check_final(mb, final, init)
    lc = [float(tb.train_iteration(img, lab)) for _ in range(2)]           # without injected noise the graph draws its own
    assert all(np.isfinite(lc))


@pytest.mark.parametrize('fixture,classes,channels,affine,conv_lu', R.FIXTURES)
def test_bf16_tracks_fp32(fixture, classes, channels, affine, conv_lu):
    """bf16 compute (fp32 accumulation, fp32 log-determinants, the factorisation in float64 either way):
    test_mcglow_gpu.py's bf16 bounds on the likelihood and on the training steps' losses."""
    from mcgen_amd.trainer import GlowTrainer
    d = R.load(fixture)
    _, init, _ = R.states(d)
    img, lab = _batch(d)
    m = _model(init, classes, channels, affine, conv_lu, torch.bfloat16)
    m.train(True)
    with torch.no_grad():
        out = m({'img': img, 'label': lab, 'noise': _noise(d, 0)})
    print('bf16 loss', float(out['loss']), float(d['losses'][0]))
    assert abs(float(out['loss']) - float(d['losses'][0])) < 2e-2
    tr = GlowTrainer(m)
    losses = [float(tr.train_iteration(img, lab, _noise(d, s))) for s in range(2)]
    print('bf16 losses', losses, d['losses'])
    for got, ref, tol in zip(losses, d['losses'], [2e-2, 3e-2]):
        assert abs(got - ref) < tol, (losses, d['losses'])
    m.train(False)
    gen = m.generate(lab)
    assert bool(torch.isfinite(gen).all()) and float(gen.abs().max()) <= 1.0


def test_create_then_generate_on_the_plain_additive_model():
    """models.utils.create (new codebooks for another number of modes) followed by generate: finite images of the right shape."""
    from mcgen_amd.config import cfg
    from mcgen_amd.models.utils import create
    fixture, classes, channels, affine, conv_lu = R.FIXTURES[2]
    d = R.load(fixture)
    _, _, final = R.states(d)
    m = _model(final, classes, channels, affine, conv_lu)
    m.train(False)
    cfg['classes_size'] = 24
    torch.manual_seed(5)
    create(m)
    assert m.blocks[0].flows[0].coupling.net[3].codebook.shape == (24, R.HIDDEN)
    lab = torch.arange(24, device='cuda')
    with torch.no_grad():
        gen = m.generate(lab)
    assert gen.shape == (24, channels, 32, 32) and bool(torch.isfinite(gen).all()) and float(gen.abs().max()) <= 1.0
    assert float((gen[0] - gen[23]).abs().max()) > 0
