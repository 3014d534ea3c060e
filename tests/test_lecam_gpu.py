"""The LeCam regulariser of the discriminator loss (trainer.FusedLeCam; lecam_lambda > 0) through the trainer, the graphs and
the driver: MCGAN against the CPU oracle with the regulariser in its D-loss line (tests/lecam_ref.OracleMCGANLeCam), CGAN
against the reference loop body on the module surface through autograd with the term added.  Fixtures, inputs and
tolerances are those of the tests this file is the counterpart of (test_gan_bce_gpu.py, and through it test_mcgan_gpu.py /
test_cgan_gpu.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
import lecam_ref as L
from test_cgan_gpu import _bn_fed_bias, _build as _build_cgan, _init_state
from test_gan_bce_gpu import SMALL, _bce_d, _bce_g, _flat_grads
from test_mcgan_gpu import _build, _oracle_grads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM, DECAY = 0.3, 0.9


def _hinge_d(d_x, d_gz):
    return torch.relu(1.0 - d_x).mean() + torch.relu(1.0 + d_gz).mean()


def _with_term(base, d_x, d_gz, lam, a_r, a_f):
    return base + lam * (((d_x - a_f) ** 2).mean() + ((d_gz - a_r) ** 2).mean())


def _lecam_state(tr):
    a_r, a_f = tr.lecam.anchors()
    return {'a_R': float(a_r), 'a_F': float(a_f), 't': int(tr.lecam.step_count)}


@pytest.mark.parametrize('loss_type', ['Hinge', 'BCE'])
def test_lecam_gradients_vs_oracle(loss_type):
    """Every discriminator parameter gradient of one D loss with the regulariser (tr.d_compute, preset anchors 0.3 / -0.2,
    start 0) on mcgan_small.npz against autograd on the CPU oracle, to test_bce_gradients_vs_oracle's bound; the loss value
    to 1e-4; the anchors after the update to the float32 recursion."""
    from oracle import mcgan_oracle as O
    from mcgen_amd.trainer import GANTrainer
    d = gu.load_npz('mcgan_small.npz')
    sd = gu.state_from_npz(d)
    img, lab = torch.from_numpy(d['img']), torch.from_numpy(d['label'])
    ind = O.one_hot(lab, 10)
    a_r, a_f, t0 = 0.3, -0.2, 4
    base = _bce_d if loss_type == 'BCE' else _hinge_d
    fake_img = torch.tanh(torch.randn(img.shape, generator=torch.Generator().manual_seed(9)))

    def loss_of(st):
        d_x = O.discriminator_forward(st, img, ind, True, cifar_layout=True)
        d_gz = O.discriminator_forward(st, fake_img, ind, True, cifar_layout=True)
        return _with_term(base(d_x, d_gz), d_x, d_gz, LAM, L.f32(a_r), L.f32(a_f)), d_x, d_gz
    ref = _oracle_grads(sd, lambda st: loss_of(st)[0])
    m = _build(*SMALL, sd)
    m.train(True)
    tr = GANTrainer(m, 10, loss_type=loss_type, lecam_lambda=LAM, lecam_decay=DECAY)
    tr.lecam.load_state_dict({'a_R': a_r, 'a_F': a_f, 'step': t0})
    loss = tr.d_compute(img.cuda(), ind.cuda(), fake_img.cuda())
    got = _flat_grads(m, 'discriminator', tr.deng, tr.grad_d)
    assert ref and set(ref) <= set(got)
    bad = []
    for k, r in ref.items():
        err = float((got[k].cpu() - r).abs().max())
        scale = float(r.abs().max()) + 1e-8
        if err > 2e-4 * scale + 1e-6:
            bad.append(f'{k}: err {err:.3e} vs scale {scale:.3e}')
    assert not bad, 'D-step mismatches:\n' + '\n'.join(bad)
    with torch.no_grad():
        want, d_x, d_gz = loss_of({k: v.clone() for k, v in sd.items()})
    assert abs(float(loss) - float(want)) < 1e-4, (float(loss), float(want))
    # the regulariser is not a no-op here: without it the loss differs
    assert abs(float(want) - float(base(d_x, d_gz))) > 1e-3
    st = _lecam_state(tr)
    assert st['t'] == t0 + 1
    assert abs(st['a_R'] - (DECAY * a_r + (1 - DECAY) * float(d_x.mean()))) < 1e-5
    assert abs(st['a_F'] - (DECAY * a_f + (1 - DECAY) * float(d_gz.mean()))) < 1e-5
    stats = {k: float(v) for k, v in tr.lecam.stats().items()}
    assert abs(stats['m_R'] - float(d_x.mean())) < 1e-5 and abs(stats['m_F'] - float(d_gz.mean())) < 1e-5
    assert abs(stats['r_t'] - float(torch.sign(d_x).mean())) < 1e-6


@pytest.mark.parametrize('loss_type,start', [('Hinge', 0), ('BCE', 0), ('Hinge', 7)])
def test_small_train_follows_the_lecam_oracle(loss_type, start, capsys):
    """Two iterations (5 D + 1 G each) of GANTrainer(lecam_lambda=...) on mcgan_small.npz against OracleMCGANLeCam run
    alongside: losses atol 1e-4 on the first iteration and 2e-3 on the second, parameters as test_small_train_losses
    compares them, anchors and t against the oracle's.  start = 7: the term switches on inside the second iteration.
    Measured on an MI355X (2026-10-21), |loss - oracle| on iteration 1 / 2: Hinge start 0 9.1e-5 / 4.5e-5, BCE start 0
    9.5e-7 / 1.2e-7, Hinge start 7 4.8e-7 / 2.2e-5."""
    from mcgen_amd.trainer import GANTrainer
    d = gu.load_npz('mcgan_small.npz')
    sd = gu.state_from_npz(d)
    img, lab = torch.from_numpy(d['img']), torch.from_numpy(d['label'])
    zs = [torch.from_numpy(z) for z in d['z'][:12]]
    oracle = L.OracleMCGANLeCam(sd, 10, LAM, decay=DECAY, start=start, loss_type=loss_type)
    ref = np.array([oracle.train_iteration(img, lab, zs[6 * it:6 * it + 6]) for it in range(2)])
    m = _build(*SMALL, sd)
    tr = GANTrainer(m, 10, loss_type=loss_type, lecam_lambda=LAM, lecam_decay=DECAY, lecam_start=start)
    got = np.array([[float(v) for v in tr.train_iteration(img.cuda(), lab.cuda(), [z.cuda() for z in zs[6 * it:6 * it + 6]])]
                    for it in range(2)])
    with capsys.disabled():
        print(f'\n[LeCam {loss_type} start={start}] |loss - oracle|: iteration 1 {np.abs(got[0] - ref[0]).max():.3e}, '
              f'iteration 2 {np.abs(got[1] - ref[1]).max():.3e}')
    np.testing.assert_allclose(got[0], ref[0], rtol=0, atol=1e-4)
    np.testing.assert_allclose(got[1], ref[1], rtol=0, atol=2e-3)
    st = _lecam_state(tr)
    assert st['t'] == oracle.lecam['t'] == 10
    # the anchors are means of logits that agree to the losses' tolerance on the second iteration
    assert abs(st['a_R'] - oracle.lecam['a_R']) < 2e-3 and abs(st['a_F'] - oracle.lecam['a_F']) < 2e-3
    got_sd = m.state_dict()
    noisy = ('linear.module.bias', 'conv.4.module.bias', 'conv.8.module.bias', 'shortcut.2.module.bias', 'running_mean')
    for k, v in oracle.sd.items():
        v = v.detach()
        if v.dtype == torch.int64:
            assert int(got_sd[k]) == int(v), k
        elif k.startswith('generator.') and k.endswith(noisy):
            assert float((got_sd[k].cpu() - v).abs().max()) < 1.5 * 3 * 2e-4 + 1e-4, k
        else:
            assert float((got_sd[k].cpu() - v).abs().max()) < 1e-3 * float(v.abs().max()) + 4e-4, k


def test_lambda_zero_reproduces_the_hinge_fixture_exactly():
    """lecam_lambda = 0 (given explicitly) is the trainer without the argument: no holder, and the two iterations' losses
    are bit for bit the default trainer's, which test_small_train_follows_the_oracle[Hinge] holds to the fixture."""
    from mcgen_amd.trainer import GANTrainer
    d = gu.load_npz('mcgan_small.npz')
    sd = gu.state_from_npz(d)
    img, lab = torch.from_numpy(d['img']).cuda(), torch.from_numpy(d['label']).cuda()
    zs = [torch.from_numpy(z).cuda() for z in d['z'][:12]]
    runs = []
    for kw in ({}, {'lecam_lambda': 0.0, 'lecam_decay': 0.5, 'lecam_start': 3}):
        tr = GANTrainer(_build(*SMALL, sd), 10, **kw)
        assert tr.lecam is None
        runs.append([[float(v) for v in tr.train_iteration(img, lab, zs[6 * it:6 * it + 6])] for it in range(2)])
    assert runs[0] == runs[1]
    np.testing.assert_allclose(runs[1][0], d['losses'][0], rtol=0, atol=1e-4)


def test_cgan_lecam_engine_follows_autograd():
    """CGAN on cgan_small.npz: the engine trainer with lecam_lambda > 0 (two separate D passes, so the stand-alone entry)
    against the reference loop body on the module surface through autograd with the term added and the anchors kept as
    the definition says.  Two iterations, losses atol 1e-4 / 2e-3, parameters as test_cgan_bce_engine_follows_autograd."""
    from mcgen_amd.trainer import GANTrainer
    d = gu.load_npz('cgan_small.npz')
    img, lab = torch.from_numpy(d['img']).cuda(), torch.from_numpy(d['label']).cuda()
    zs = [torch.from_numpy(z).cuda() for z in d['z']]
    ma = _build_cgan('CIFAR10', 10, [32] * 4, [16] * 4, _init_state(d))
    opt = {k: torch.optim.Adam(getattr(ma, k).parameters(), lr=2e-4, betas=(0.5, 0.999)) for k in ('generator', 'discriminator')}
    zi = iter(zs)
    ma.train(True)
    ref, s = [], L.fresh_state()
    for _ in range(2):
        for _ in range(5):
            opt['discriminator'].zero_grad(); opt['generator'].zero_grad()
            d_x = ma.discriminate(img, lab)
            fake = ma.generate(lab, next(zi))
            d_gz = ma.discriminate(fake.detach(), lab)
            d_loss = _with_term(_hinge_d(d_x, d_gz), d_x, d_gz, LAM, s['a_R'], s['a_F'])
            m_r, m_f = float(d_x.mean()), float(d_gz.mean())
            s['a_R'], s['a_F'] = (m_r, m_f) if s['t'] == 0 else (DECAY * s['a_R'] + (1 - DECAY) * m_r, DECAY * s['a_F'] + (1 - DECAY) * m_f)
            s['t'] += 1
            d_loss.backward()
            opt['discriminator'].step()
        opt['discriminator'].zero_grad(); opt['generator'].zero_grad()
        g_loss = -ma.discriminate(ma.generate(lab, next(zi)), lab).mean()
        g_loss.backward()
        opt['generator'].step()
        ref.append((float(d_loss.detach()), float(g_loss.detach())))
    ref_sd = {k: v.detach().cpu().clone() for k, v in ma.state_dict().items()}
    me = _build_cgan('CIFAR10', 10, [32] * 4, [16] * 4, _init_state(d))
    tr = GANTrainer(me, 10, lecam_lambda=LAM, lecam_decay=DECAY)
    got = [tuple(float(v) for v in tr.train_iteration(img, lab, zs[6 * i:6 * i + 6])) for i in range(2)]
    np.testing.assert_allclose(got[0], ref[0], rtol=0, atol=1e-4)
    np.testing.assert_allclose(got[1], ref[1], rtol=0, atol=2e-3)
    assert abs(ref[0][0] - float(d['losses'][0][0])) > 1e-3              # (not the plain hinge loss)
    st = _lecam_state(tr)
    assert st['t'] == 10 and abs(st['a_R'] - s['a_R']) < 2e-3 and abs(st['a_F'] - s['a_F']) < 2e-3
    sd = me.state_dict()
    for k, v in ref_sd.items():
        if v.dtype == torch.int64:
            assert int(sd[k]) == int(v), k
        else:
            tol = 8e-4 if _bn_fed_bias(k) else 1e-3 * float(v.abs().max()) + 4e-4
            assert float((sd[k].cpu() - v).abs().max()) < tol, k


@pytest.mark.parametrize('model', ['mcgan', 'cgan'])
def test_graphed_lecam_matches_eager(model):
    """GraphedGANTrainer(lecam_lambda > 0): the capture leaves model and LeCam state as it found them; three replayed
    iterations with injected latents against the eager trainer from the same state, to test_graphed_bce_matches_eager's
    tolerances (losses 1e-4 on the first iteration, 2e-3 afterwards; state 1e-6 + 1e-5 max |v|), anchors and t included;
    the graphs hold the regulariser's launches (the losses are not the plain ones); a changed lambda, decay or start raises."""
    from mcgen_amd.trainer import GANTrainer, GraphedGANTrainer
    d = gu.load_npz(f'{model}_small.npz')
    sd0 = gu.state_from_npz(d) if model == 'mcgan' else _init_state(d)
    build = (lambda: _build(*SMALL, sd0)) if model == 'mcgan' else (lambda: _build_cgan('CIFAR10', 10, [32] * 4, [16] * 4, sd0))
    img, lab = torch.from_numpy(d['img']).cuda(), torch.from_numpy(d['label']).cuda()
    zs = [z.cuda() for z in gu.latent_batches(18, img.shape[0], 128, seed=5)]
    preset = {'a_R': 0.3, 'a_F': -0.2, 'step': 2}
    kw = dict(lecam_lambda=LAM, lecam_decay=DECAY, lecam_start=4)       # (on from the third D update of the first iteration)
    mg = build()
    tg = GraphedGANTrainer(mg, 10, **kw)
    tg.lecam.load_state_dict(preset)
    before = tg.lecam.state.clone()
    tg.capture(img, lab, warmup=1)
    torch.cuda.synchronize()
    for k, v in mg.state_dict().items():                    # capture's warm-up updates were rolled back
        assert torch.equal(v.cpu(), sd0[k]), k
    assert torch.equal(tg.lecam.state, before), 'capture advanced the LeCam state'
    l_g = np.array([[float(v) for v in tg.train_iteration(img, lab, zs[6 * it:6 * it + 6])] for it in range(3)])
    me = build()
    te = GANTrainer(me, 10, **kw)
    te.lecam.load_state_dict(preset)
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
    s_g, s_e = _lecam_state(tg), _lecam_state(te)
    assert s_g['t'] == s_e['t'] == 17
    for k in ('a_R', 'a_F'):
        assert abs(s_g[k] - s_e[k]) <= 1e-6 + 1e-5 * abs(s_e[k]), (k, s_g, s_e)
    mh = build()
    l_h = [float(v) for v in GANTrainer(mh, 10).train_iteration(img, lab, zs[:6])]
    assert abs(l_h[0] - l_g[0][0]) > 1e-3
    for name, value in (('lam', 0.5), ('decay', 0.5), ('start', 1)):
        old = getattr(tg.lecam, name)
        setattr(tg.lecam, name, value)
        with pytest.raises(ValueError, match='Not valid LeCam regulariser'):
            tg.train_iteration(img, lab, zs[:6])
        setattr(tg.lecam, name, old)
    assert _lecam_state(tg) == s_g                           # the refused calls launched nothing


@pytest.mark.parametrize('model', ['mcgan', 'cgan'])
def test_regulariser_adds_no_launch(model):
    """Kernel launches of one eager iteration (torch.profiler, as tools/bench_gan_loss.py counts them) with lambda > 0
    equal those with lambda = 0."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        from bench_cgan import _launches
    finally:
        sys.path.pop(0)
    from mcgen_amd.trainer import GANTrainer
    d = gu.load_npz(f'{model}_small.npz')
    sd0 = gu.state_from_npz(d) if model == 'mcgan' else _init_state(d)
    build = (lambda: _build(*SMALL, sd0)) if model == 'mcgan' else (lambda: _build_cgan('CIFAR10', 10, [32] * 4, [16] * 4, sd0))
    img, lab = torch.from_numpy(d['img']).cuda(), torch.from_numpy(d['label']).cuda()
    counts = {}
    for lam in (0.0, LAM):
        tr = GANTrainer(build(), 10, lecam_lambda=lam)
        tr.train_iteration(img, lab)                         # (first launches load code objects)
        counts[lam] = _launches(lambda: tr.train_iteration(img, lab))
    assert counts[0.0] is not None and counts[0.0] > 50, counts
    assert counts[LAM] == counts[0.0], counts


def test_constructor_refusals_on_the_device():
    from mcgen_amd.trainer import GANTrainer, GraphedGANTrainer
    m = _build(*SMALL)
    for cls in (GANTrainer, GraphedGANTrainer):
        with pytest.raises(ValueError, match='lecam_lambda > 0 runs on one GPU'):
            cls(m, 10, lecam_lambda=0.3, world_size=2)
        with pytest.raises(ValueError, match='Not valid LeCam regulariser'):
            cls(m, 10, lecam_lambda=0.3, lecam_decay=1.0)
    tr = GANTrainer(m, 10, lecam_lambda=0.3)
    assert tr.lecam.hyper() == (0.3, 0.99, 0) and tr._hyper()[-1] == ('lecam', 0.3, 0.99, 0)
    assert GANTrainer(m, 10).lecam is None


def _driver(tmp_path, *flags):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    return subprocess.run([sys.executable, os.path.join(ROOT, 'compat', 'train_gan.py'), '--data_name', 'CIFAR10',
                           '--model_name', 'mcgan', '--control_name', '0.5', '--engine', 'fused', '--synthetic_size', '128',
                           '--generate_per_mode', '1', '--output_dir', './output', *flags],
                          cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)


def _read_checkpoint(tmp_path):
    path = tmp_path / 'output' / 'model' / '0_CIFAR10_label_mcgan_0.5_checkpoint.pt'
    assert path.exists()
    code = r'''
import sys, torch
sys.path[:0] = [{compat!r}, {root!r}]
import logger  # noqa: F401
ck = torch.load({path!r}, map_location='cpu', weights_only=False)
print('KEYS', sorted(ck))
print('LECAM', ck.get('lecam'))
'''.format(compat=os.path.join(ROOT, 'compat'), root=ROOT, path=str(path))
    r = subprocess.run([sys.executable, '-c', code], cwd=tmp_path, env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    keys = eval(re.search(r'KEYS (.*)', r.stdout)[1])
    lecam = eval(re.search(r'LECAM (.*)', r.stdout)[1])
    return keys, lecam


def test_driver_one_epoch_lecam_then_resume(tmp_path):
    """compat/train_gan.py --lecam_lambda 0.3 --engine fused for one epoch on the smallest synthetic set the driver takes
    (one batch of 128): the log carries the LeCam line, the checkpoint the 'lecam' key (5 updates); a second epoch
    resumes with the same anchors (the line of epoch 2 starts from them: t goes on to 10).  --engine autograd refuses."""
    r = _driver(tmp_path, '--lecam_lambda', '0.3', '--lecam_decay', '0.9', '--num_epochs', '1')
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if 'LeCam: a_R' in ln]
    assert len(line) == 1, r.stdout[-2000:]
    a_r, a_f, r_t = (float(v) for v in re.search(r'LeCam: a_R (\S+) a_F (\S+) r_t (\S+)', line[0]).groups())
    assert np.isfinite([a_r, a_f, r_t]).all() and -1.0 <= r_t <= 1.0
    keys, lecam = _read_checkpoint(tmp_path)
    assert 'lecam' in keys and lecam['step'] == 5 and (lecam['lambda'], lecam['decay'], lecam['start']) == (0.3, 0.9, 0)
    assert abs(lecam['a_R'] - a_r) < 1e-4 and abs(lecam['a_F'] - a_f) < 1e-4
    r = _driver(tmp_path, '--lecam_lambda', '0.3', '--lecam_decay', '0.9', '--num_epochs', '2', '--resume_mode', '1')
    assert r.returncode == 0 and 'Resume from 2' in r.stdout and 'No LeCam state' not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    keys, again = _read_checkpoint(tmp_path)
    assert again['step'] == 10
    # five more decayed updates from the resumed anchors: had they started fresh, update 0 would have copied the mean
    assert again['a_R'] != lecam['a_R']
    r = _driver(tmp_path, '--lecam_lambda', '0.3', '--engine', 'autograd', '--num_epochs', '1')
    assert r.returncode != 0 and '--lecam_lambda needs --engine fused' in r.stderr


def test_driver_without_the_flags_has_neither(tmp_path):
    r = _driver(tmp_path, '--num_epochs', '1')
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'LeCam' not in r.stdout
    keys, lecam = _read_checkpoint(tmp_path)
    assert lecam is None and keys == ['cfg', 'epoch', 'logger', 'model_dict', 'optimizer_dict', 'scheduler_dict']
    # a checkpoint without the key resumes a run with the flag, with fresh state, and says so
    r = _driver(tmp_path, '--lecam_lambda', '0.3', '--num_epochs', '2', '--resume_mode', '1')
    assert r.returncode == 0 and 'No LeCam state' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    keys, lecam = _read_checkpoint(tmp_path)
    assert lecam['step'] == 5
