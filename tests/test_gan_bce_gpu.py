"""cfg['loss_type'] = 'BCE' (train_gan.py:148-152,168-170) through the trainer, the graphs and the driver, for MCGAN against
the CPU oracle with the BCE loss lines (tests/gan_loss_ref.OracleMCGANBCE) and for CGAN against the same loop on the module
surface through autograd.  The fixtures, inputs and tolerances are those of the hinge tests they mirror
(test_mcgan_gpu.py: test_gradients_vs_oracle, test_small_train_losses, test_graphed_trainer_matches_eager;
test_cgan_gpu.py: test_small_train_losses_and_state, test_driver_one_epoch_then_generate)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gan_loss_ref as G
import golden_util as gu
from test_cgan_gpu import _bn_fed_bias, _build as _build_cgan, _init_state
from test_mcgan_gpu import _build, _oracle_grads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ([32] * 4, [16] * 4, 10, 'CIFAR10')


def _bce_d(d_x, d_gz):
    """train_gan.py:149-152."""
    n = d_x.size(0)
    return F.binary_cross_entropy_with_logits(d_x, torch.ones((n, 1), device=d_x.device)) + \
        F.binary_cross_entropy_with_logits(d_gz, torch.zeros((n, 1), device=d_x.device))


def _bce_g(d_gz):
    """train_gan.py:169-170."""
    return F.binary_cross_entropy_with_logits(d_gz, torch.ones((d_gz.size(0), 1), device=d_gz.device))


def _flat_grads(model, part, engine, flat):
    """The trainer's flat gradient buffer split along the engine's flat parameter order -> {state_dict key: gradient}."""
    name_of = {id(p): f'{part}.{k}' for k, p in getattr(model, part).named_parameters()}
    return {name_of[id(p)]: engine.flat_p.view_of(flat, p) for p in engine.flat_p.tensors}


def test_bce_gradients_vs_oracle():
    """Every parameter gradient of one BCE discriminator loss (tr.d_compute) and one BCE generator loss (tr.g_compute) of
    mcgan_small.npz against autograd on the CPU oracle with the BCE expressions, to test_gradients_vs_oracle's bound."""
    from oracle import mcgan_oracle as O
    from mcgen_amd.trainer import GANTrainer
    d = gu.load_npz('mcgan_small.npz')
    sd = gu.state_from_npz(d)
    img, lab = torch.from_numpy(d['img']), torch.from_numpy(d['label'])
    z = torch.from_numpy(d['z'][0])
    ind = O.one_hot(lab, 10)

    def check(got, ref, what):
        bad = []
        for k, r in ref.items():
            g = got[k].cpu()
            err = float((g - r).abs().max())
            scale = float(r.abs().max()) + 1e-8
            if err > 2e-4 * scale + 1e-6:
                bad.append(f'{k}: err {err:.3e} vs scale {scale:.3e}')
        assert not bad, what + ' mismatches:\n' + '\n'.join(bad)

    fake_img = torch.tanh(torch.randn(img.shape, generator=torch.Generator().manual_seed(9)))
    ref = _oracle_grads(sd, lambda st: _bce_d(O.discriminator_forward(st, img, ind, True, cifar_layout=True),
                                               O.discriminator_forward(st, fake_img, ind, True, cifar_layout=True)))
    m = _build(*SMALL, sd)
    m.train(True)
    tr = GANTrainer(m, 10, loss_type='BCE')
    loss = tr.d_compute(img.cuda(), ind.cuda(), fake_img.cuda())
    got = _flat_grads(m, 'discriminator', tr.deng, tr.grad_d)
    assert ref and set(ref) <= set(got)
    check(got, ref, 'D-step')
    with torch.no_grad():
        st = {k: v.clone() for k, v in sd.items()}
        want = float(_bce_d(O.discriminator_forward(st, img, ind, True, cifar_layout=True),
                            O.discriminator_forward(st, fake_img, ind, True, cifar_layout=True)))
    assert abs(float(loss) - want) < 1e-4, (float(loss), want)
    # the generator loss through D, from the same initial state (u, v, running statistics)
    ref = _oracle_grads(sd, lambda st: _bce_g(O.discriminator_forward(st, O.generator_forward(st, z, ind, True), ind, True,
                                                                      cifar_layout=True)))
    ref = {k: v for k, v in ref.items() if k.startswith('generator.')}
    m = _build(*SMALL, sd)
    m.train(True)
    tr = GANTrainer(m, 10, loss_type='BCE')
    tr.g_compute(ind.cuda(), z.cuda())
    got = _flat_grads(m, 'generator', tr.geng, tr.grad_g)
    assert ref and set(ref) <= set(got)
    check(got, ref, 'G-step')


@pytest.mark.parametrize('loss_type', ['Hinge', 'BCE'])
def test_small_train_follows_the_oracle(loss_type, capsys):
    """Two iterations (5 D + 1 G each) of GANTrainer(loss_type=...) on mcgan_small.npz -- test_small_train_losses' state,
    images, labels and latents -- against the CPU oracle run alongside: the unmodified OracleMCGAN for 'Hinge' (the harness
    itself), OracleMCGANBCE for 'BCE'.  Losses atol 1e-4 on the first iteration and 2e-3 on the second, parameters as
    test_small_train_losses compares them.  Measured on an MI355X (2026-10-21), |loss - oracle| on iteration 1 / 2:
    Hinge 4.8e-7 / 2.6e-5, BCE 2.4e-7 / 1.2e-7; worst parameter error over its bound: Hinge 0.85, BCE 0.02 (BCE has no
    rounding-decided zero gradients for Adam to amplify: every sample's derivative is non-zero)."""
    from oracle import mcgan_oracle as O
    from mcgen_amd.trainer import GANTrainer
    d = gu.load_npz('mcgan_small.npz')
    sd = gu.state_from_npz(d)
    img, lab = torch.from_numpy(d['img']), torch.from_numpy(d['label'])
    zs = [torch.from_numpy(z) for z in d['z'][:12]]
    oracle = (G.OracleMCGANBCE if loss_type == 'BCE' else O.OracleMCGAN)(sd, classes=10)
    ref = np.array([oracle.train_iteration(img, lab, zs[6 * it:6 * it + 6]) for it in range(2)])
    m = _build(*SMALL, sd)
    tr = GANTrainer(m, 10, loss_type=loss_type)
    got = np.array([[float(v) for v in tr.train_iteration(img.cuda(), lab.cuda(), [z.cuda() for z in zs[6 * it:6 * it + 6]])]
                    for it in range(2)])
    with capsys.disabled():
        print(f'\n[{loss_type}] |loss - oracle|: iteration 1 {np.abs(got[0] - ref[0]).max():.3e}, '
              f'iteration 2 {np.abs(got[1] - ref[1]).max():.3e}')
    if loss_type == 'Hinge':
        np.testing.assert_allclose(ref[0], d['losses'][0], rtol=0, atol=1e-4)     # the oracle follows the reference's fixture
    np.testing.assert_allclose(got[0], ref[0], rtol=0, atol=1e-4)
    np.testing.assert_allclose(got[1], ref[1], rtol=0, atol=2e-3)
    got_sd = m.state_dict()
    noisy = ('linear.module.bias', 'conv.4.module.bias', 'conv.8.module.bias', 'shortcut.2.module.bias', 'running_mean')
    worst = 0.0
    for k, v in oracle.sd.items():
        v = v.detach()
        if v.dtype == torch.int64:
            assert int(got_sd[k]) == int(v), k
        elif k.startswith('generator.') and k.endswith(noisy):
            assert float((got_sd[k].cpu() - v).abs().max()) < 1.5 * 3 * 2e-4 + 1e-4, k
        else:
            err = float((got_sd[k].cpu() - v).abs().max())
            worst = max(worst, err / (1e-3 * float(v.abs().max()) + 4e-4))
            assert err < 1e-3 * float(v.abs().max()) + 4e-4, k
    with capsys.disabled():
        print(f'[{loss_type}] worst parameter error / bound: {worst:.3f}')


def test_cgan_bce_engine_follows_autograd():
    """CGAN on cgan_small.npz: the engine trainer with loss_type='BCE' against the reference loop body on the module surface
    through autograd with the BCE expressions (the 'autograd' path of test_small_train_losses_and_state).  Two iterations,
    losses atol 1e-4 / 2e-3, parameters as that test compares them."""
    from mcgen_amd.trainer import GANTrainer
    d = gu.load_npz('cgan_small.npz')
    img, lab = torch.from_numpy(d['img']).cuda(), torch.from_numpy(d['label']).cuda()
    zs = [torch.from_numpy(z).cuda() for z in d['z']]
    # the reference loop body (train_gan.py:139-176)
    ma = _build_cgan('CIFAR10', 10, [32] * 4, [16] * 4, _init_state(d))
    opt = {k: torch.optim.Adam(getattr(ma, k).parameters(), lr=2e-4, betas=(0.5, 0.999)) for k in ('generator', 'discriminator')}
    zi = iter(zs)
    ma.train(True)
    ref = []
    for _ in range(2):
        for _ in range(5):
            opt['discriminator'].zero_grad(); opt['generator'].zero_grad()
            d_x = ma.discriminate(img, lab)
            fake = ma.generate(lab, next(zi))
            d_loss = _bce_d(d_x, ma.discriminate(fake.detach(), lab))
            d_loss.backward()
            opt['discriminator'].step()
        opt['discriminator'].zero_grad(); opt['generator'].zero_grad()
        g_loss = _bce_g(ma.discriminate(ma.generate(lab, next(zi)), lab))
        g_loss.backward()
        opt['generator'].step()
        ref.append((float(d_loss.detach()), float(g_loss.detach())))
    ref_sd = {k: v.detach().cpu().clone() for k, v in ma.state_dict().items()}
    me = _build_cgan('CIFAR10', 10, [32] * 4, [16] * 4, _init_state(d))
    tr = GANTrainer(me, 10, loss_type='BCE')
    got = [tuple(float(v) for v in tr.train_iteration(img, lab, zs[6 * i:6 * i + 6])) for i in range(2)]
    np.testing.assert_allclose(got[0], ref[0], rtol=0, atol=1e-4)
    np.testing.assert_allclose(got[1], ref[1], rtol=0, atol=2e-3)
    assert abs(ref[0][0] - float(d['losses'][0][0])) > 1e-3              # (not the hinge loss)
    sd = me.state_dict()
    for k, v in ref_sd.items():
        if v.dtype == torch.int64:
            assert int(sd[k]) == int(v), k
        else:
            tol = 8e-4 if _bn_fed_bias(k) else 1e-3 * float(v.abs().max()) + 4e-4
            assert float((sd[k].cpu() - v).abs().max()) < tol, k


@pytest.mark.parametrize('model', ['mcgan', 'cgan'])
def test_graphed_bce_matches_eager(model):
    """GraphedGANTrainer(loss_type='BCE'): capture, three replayed iterations with injected latents, against the eager
    trainer from the same state, to test_graphed_trainer_matches_eager's tolerances (losses 1e-4 on the first iteration,
    2e-3 afterwards; state 1e-6 + 1e-5 max |v|); and the graphs hold the BCE launches: the losses are not the hinge ones."""
    from mcgen_amd.trainer import GANTrainer, GraphedGANTrainer
    d = gu.load_npz(f'{model}_small.npz')
    sd0 = gu.state_from_npz(d) if model == 'mcgan' else _init_state(d)
    build = (lambda: _build(*SMALL, sd0)) if model == 'mcgan' else (lambda: _build_cgan('CIFAR10', 10, [32] * 4, [16] * 4, sd0))
    img, lab = torch.from_numpy(d['img']).cuda(), torch.from_numpy(d['label']).cuda()
    zs = [z.cuda() for z in gu.latent_batches(18, img.shape[0], 128, seed=5)]
    mg = build()
    tg = GraphedGANTrainer(mg, 10, loss_type='BCE')
    tg.capture(img, lab, warmup=1)
    torch.cuda.synchronize()
    for k, v in mg.state_dict().items():                    # capture's warm-up updates were rolled back
        assert torch.equal(v.cpu(), sd0[k]), k
    l_g = np.array([[float(v) for v in tg.train_iteration(img, lab, zs[6 * it:6 * it + 6])] for it in range(3)])
    me = build()
    te = GANTrainer(me, 10, loss_type='BCE')
    l_e = np.array([[float(v) for v in te.train_iteration(img, lab, zs[6 * it:6 * it + 6])] for it in range(3)])
    np.testing.assert_allclose(l_g[0], l_e[0], rtol=0, atol=1e-4)
    np.testing.assert_allclose(l_g[1:], l_e[1:], rtol=0, atol=2e-3)
    sd_g, sd_e = mg.state_dict(), me.state_dict()
    for k, v in sd_e.items():
        if v.dtype == torch.int64:
            assert int(sd_g[k]) == int(v), k
        else:
            assert float((sd_g[k] - v).abs().max()) <= 1e-6 + 1e-5 * float(v.abs().max()), k
    assert int(tg.opt_d.step_count) == 15 and int(tg.opt_g.step_count) == 3
    mh = build()
    l_h = [float(v) for v in GANTrainer(mh, 10).train_iteration(img, lab, zs[:6])]
    assert abs(l_h[0] - l_g[0][0]) > 1e-3 and abs(l_h[1] - l_g[0][1]) > 1e-3
    assert (l_g > 0).all()                                  # (a BCE loss is positive; the hinge G loss need not be)


def test_constructor_refuses_an_unknown_loss_type():
    from mcgen_amd.trainer import GANTrainer, GraphedGANTrainer
    m = _build(*SMALL)
    for cls in (GANTrainer, GraphedGANTrainer):
        with pytest.raises(ValueError, match='Not valid loss type'):
            cls(m, 10, loss_type='WGAN')
    assert GANTrainer(m, 10).loss_type == 'Hinge'


def test_driver_one_epoch_bce(tmp_path):
    """compat/train_gan.py --loss_type BCE --model_name mcgan --engine fused for one epoch on the smallest synthetic set the
    driver takes (one batch of 128): finite losses in the log line, cfg['loss_type'] == 'BCE' in the checkpoint, the tag
    unchanged."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'compat', 'train_gan.py'), '--data_name', 'CIFAR10',
                        '--model_name', 'mcgan', '--control_name', '0.5', '--engine', 'fused', '--loss_type', 'BCE',
                        '--num_epochs', '1', '--synthetic_size', '128', '--generate_per_mode', '1', '--output_dir', './output'],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'Experiment: 0_CIFAR10_label_mcgan_0.5' in r.stdout
    line = [ln for ln in r.stdout.splitlines() if 'Loss_D:' in ln]
    assert len(line) == 1, r.stdout[-2000:]
    vals = {k: float(v) for k, v in re.findall(r'(Loss(?:_D|_G)?): (\S+)', line[0])}
    assert set(vals) == {'Loss', 'Loss_D', 'Loss_G'} and all(np.isfinite(v) for v in vals.values()), line[0]
    assert vals['Loss_D'] > 0 and vals['Loss_G'] > 0
    path = tmp_path / 'output' / 'model' / '0_CIFAR10_label_mcgan_0.5_checkpoint.pt'
    assert path.exists()
    code = r'''
import sys, torch
sys.path[:0] = [{compat!r}, {root!r}]
import logger  # noqa: F401
ck = torch.load({path!r}, map_location='cpu', weights_only=False)
print('loss_type', ck['cfg']['loss_type'], ck['epoch'])
'''.format(compat=os.path.join(ROOT, 'compat'), root=ROOT, path=str(path))
    r = subprocess.run([sys.executable, '-c', code], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'loss_type BCE 2' in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
