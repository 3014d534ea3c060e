"""VQ-VAE training on the HIP path (train_vqvae.py): the quantiser's training-step kernels against an fp64 restatement
of modules.py:18-43, the tanh + MSE loss kernel, the model's step 0 / 3 steps / eval forward against the reference
fixtures (tests/golden/vqvae_train_small.npz, vqvae_train_full_digest.npz), the graphed trainer, the autograd bridge,
bf16, and the train_vqvae -> train_pixelcnn pipeline of the compat drivers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
import pixel_ops_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = {'hidden_size': [16, 16], 'num_res_block': 2, 'embedding_size': 8, 'num_embedding': 64, 'vq_commit': 0.25}
FULL = {'hidden_size': [128, 128], 'num_res_block': 2, 'embedding_size': 64, 'num_embedding': 512, 'vq_commit': 0.25}


def _rel(a, b):
    a = torch.as_tensor(a).double().cpu()
    b = b.double().cpu() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _model(vq, sd=None, dtype=torch.float32):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name='vqvae', device='cuda', data_shape=[3, 32, 32], compute_dtype='float32')
    cfg['vqvae'] = dict(vq)
    m = models.vqvae()
    if sd is not None:
        m.load_state_dict(sd)
    m = m.cuda().set_compute_dtype(dtype)
    m.train(True)
    return m


def _full_state(d):
    from mcgen_amd import models  # noqa: F401
    m = _model(FULL)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = gu.procedural_state_generic(shapes, seed=7301)
    emb = torch.from_numpy(d['q_embedding'])
    sd['quantizer.embedding'] = emb.clone(); sd['quantizer.embedding_mean'] = emb.clone()
    sd['quantizer.cluster_size'] = torch.zeros(512)
    return sd


# ---- kernels ------------------------------------------------------------------------------------------------------
def _vq_case(d, k, p, seed):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(d, k, generator=g, dtype=torch.float64)
    codes = torch.randint(0, k, (p,), generator=g)
    codes[torch.randperm(p, generator=g)[:p // 2 + 7]] = 3                # one code takes more than half of the pixels
    codes[codes == 5] = 6                                                   # one code is never hit
    feat = emb[:, codes].t() + 1e-3 * torch.randn(p, d, generator=g, dtype=torch.float64)
    cs0 = torch.rand(k, generator=g, dtype=torch.float64) * 4
    mean0 = emb * (cs0 + 1e-5)
    return emb, codes, feat, cs0, mean0


@pytest.mark.parametrize('d,k', [(8, 64), (64, 512)])
def test_vq_step_kernel_matches_fp64(d, k):
    from mcgen_amd import ops
    from mcgen_amd.modules import VectorQuantization
    p, decay, eps, commit = 1000, 0.99, 1e-5, 0.25
    emb, codes, feat, cs0, mean0 = _vq_case(d, k, p, seed=d + k)
    vq = VectorQuantization(d, k).cuda()
    runs = []
    for _ in range(2):
        vq.embedding.copy_(emb.float()); vq.cluster_size.copy_(cs0.float()); vq.embedding_mean.copy_(mean0.float())
        f = feat.float().cuda().reshape(p, 1, 1, d).contiguous()
        idx = vq._nearest(f)
        q, gq, diff, counts = ops.vq_step(f, idx, vq.embedding, d, torch.float32, coef=commit * 2 / (p * d), want_grad=True,
                                          train=True, cluster_size=vq.cluster_size, embedding_mean=vq.embedding_mean,
                                          want_counts=True)
        torch.cuda.synchronize()
        runs.append([t.detach().clone().cpu() for t in (idx, q, gq, diff, counts, vq.cluster_size, vq.embedding_mean, vq.embedding)])
    idx, q, gq, diff, counts, cs, em, e = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)                                            # bit-identical reruns: no float atomics
    # fp64 restatement of modules.py:18-43 (pixel_ops_ref.vq_step)
    f64 = feat.float().double()
    assert torch.equal(idx.view(-1), codes)
    r = R.vq_step(f64, codes, emb.float(), cs0.float(), mean0.float(), decay, 1 - decay, eps, commit)
    cnt, q_ref, cs_ref, em_ref, e_ref, diff_ref, g_ref = (r[k] for k in ('counts', 'q', 'cs', 'em', 'e', 'diff', 'g'))
    assert torch.equal(counts.double(), cnt) and cnt[5] == 0 and cnt[3] > p // 2
    assert _rel(q.view(p, d), q_ref) == 0.0
    assert _rel(cs, cs_ref) < 1e-6 and _rel(em, em_ref) < 1e-6 and _rel(e, e_ref) < 1e-6
    assert abs(float(diff) - float(diff_ref)) <= 1e-6 * float(diff_ref)
    assert _rel(gq.view(p, d), g_ref) < 1e-6


def test_mse_tanh_kernel_matches_autograd():
    from mcgen_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 3, 32, 32, generator=g, dtype=torch.float64)
    t = torch.rand(4, 3, 32, 32, generator=g, dtype=torch.float64) * 2 - 1
    xn = ops.to_nhwc(x.float().cuda(), torch.float32)
    tn = ops.to_nhwc(t.float().cuda(), torch.float32, xn.shape[-1])
    numel = float(x.numel())
    dec, sse, dx = ops.mse_tanh(xn, tn, 3, 2.0 / numel, True)
    xr = x.float().double().requires_grad_(True)
    decr = torch.tanh(xr)
    loss = torch.nn.functional.mse_loss(decr, t.float().double())
    loss.backward()
    assert _rel(ops.to_nchw(dec, 3), decr.detach()) < 1e-6
    assert abs(float(sse) / numel - float(loss)) < 1e-6 * float(loss)
    assert _rel(ops.to_nchw(dx, 3), xr.grad) < 1e-6


# ---- model against the reference fixture ---------------------------------------------------------------------------
def _step0(m, img):
    from mcgen_amd.trainer import VQVAETrainer
    tr = VQVAETrainer(m)
    tr._bind_grads()
    eng = m._engine()
    tape = []
    with torch.no_grad():
        out = eng.forward(img, True, tape, want_grad=True)
        eng.backward(tape)
    torch.cuda.synchronize()
    return tr, out


def test_vqvae_small_step0_and_steps_match_reference():
    d = gu.load_npz('vqvae_train_small.npz')
    img = torch.from_numpy(d['img']).cuda()
    m = _model(SMALL, gu.state_from_npz(d))
    tr, out = _step0(m, img)
    assert abs(float(out['loss']) - float(d['loss0'])) < 1e-5
    assert abs(float(out['mse']) - float(d['mse0'])) < 1e-5 and abs(float(out['diff']) - float(d['vq0'])) < 1e-5
    code, ref = out['code'].cpu(), torch.from_numpy(d['code0'])
    decisive = torch.from_numpy(d['dist_margin0'] > 1e-4)
    assert torch.equal(code[decisive], ref[decisive]) and float((code == ref).float().mean()) >= 0.97
    assert _rel(out['img'], d['img0']) < 1e-4
    for k, p in m.named_parameters():
        gr = torch.from_numpy(d['grad0/' + k])
        bound = 5e-4 * float(gr.abs().max()) + 2e-7
        assert float((p.grad.cpu() - gr).abs().max()) <= bound, k
    for k, b in m.named_buffers():
        if k.endswith('num_batches_tracked'):
            assert int(b) == int(d['buf1/' + k]), k
        else:
            assert _rel(b, d['buf1/' + k]) < 1e-5, k
    # 3 loop-body steps from the initial state on the eager trainer
    m = _model(SMALL, gu.state_from_npz(d))
    from mcgen_amd.trainer import VQVAETrainer
    tr = VQVAETrainer(m)
    losses = [float(tr.train_iteration(img)) for _ in range(3)]
    assert max(abs(a - b) for a, b in zip(losses, d['losses'])) < 2e-3, (losses, d['losses'])
    # eval-mode forward on the reference's final state (train_vqvae.py::test)
    mf = _model(SMALL, gu.state_from_npz(d, 'sd_final/'))
    mf.train(False)
    with torch.no_grad():
        ev = mf({'img': img})
    assert abs(float(ev['loss']) - float(d['eval_loss'])) < 1e-5
    assert float((ev['code'].cpu() == torch.from_numpy(d['eval_code'])).float().mean()) >= 0.97
    # training-mode encode stays refused (training goes through forward / the trainer)
    with pytest.raises(NotImplementedError):
        mf.train(True).encode(img)


def test_vqvae_graphed_trainer_equals_eager_and_bridge_gradients():
    from mcgen_amd.trainer import VQVAETrainer
    d = gu.load_npz('vqvae_train_small.npz')
    img = torch.from_numpy(d['img']).cuda()
    ma, mb = _model(SMALL, gu.state_from_npz(d)), _model(SMALL, gu.state_from_npz(d))
    ta, tb = VQVAETrainer(ma), VQVAETrainer(mb)
    tb.capture(img)
    sd0 = gu.state_from_npz(d)
    for k, v in mb.state_dict().items():                                    # capture did not advance training
        assert torch.equal(v.cpu(), sd0[k]), k
    la = [float(ta.train_iteration(img)) for _ in range(3)]
    lb = [float(tb.train_iteration(img)) for _ in range(3)]
    assert max(abs(a - b) for a, b in zip(la, lb)) < 1e-6, (la, lb)
    sa, sb = ma.state_dict(), mb.state_dict()
    for k in sa:
        if sa[k].is_floating_point():
            assert _rel(sb[k], sa[k]) < 1e-6, k
        else:
            assert torch.equal(sa[k], sb[k]), k
    # a batch of another size (the loader's short final batch) runs the eager step next to the captured graph
    assert np.isfinite(float(tb.train_iteration(img[:5])))
    # autograd bridge: model(input)['loss'].backward() gives the trainer's gradients
    m1, m2 = _model(SMALL, gu.state_from_npz(d)), _model(SMALL, gu.state_from_npz(d))
    out = m1({'img': img})
    out['loss'].backward()
    t2, _ = _step0(m2, img)
    for (k, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert _rel(p1.grad, p2.grad) < 1e-6, k
    assert set(out) == {'loss', 'code', 'img'}
    # training mode under no_grad: forward only, BN running statistics and the EMA buffers still move
    m3 = _model(SMALL, gu.state_from_npz(d))
    with torch.no_grad():
        m3({'img': img})
    assert _rel(m3.quantizer.cluster_size, d['buf1/quantizer.cluster_size']) < 1e-5
    assert int(m3.encoder.blocks[1].num_batches_tracked) == 1


def test_vqvae_bf16_tracks_fp32_fixture():
    from mcgen_amd.trainer import VQVAETrainer
    d = gu.load_npz('vqvae_train_small.npz')
    img = torch.from_numpy(d['img']).cuda()
    m = _model(SMALL, gu.state_from_npz(d), dtype=torch.bfloat16)
    with torch.no_grad():
        out = m._engine().forward(img, False)
    tr = VQVAETrainer(_model(SMALL, gu.state_from_npz(d), dtype=torch.bfloat16))
    tr.capture(img)
    losses = [float(tr.train_iteration(img)) for _ in range(3)]
    assert abs(losses[0] - float(d['loss0'])) < 1e-2, losses
    assert max(abs(a - b) for a, b in zip(losses, d['losses'])) < 2e-2, (losses, d['losses'])
    assert np.isfinite(float(out['loss']))


def test_vqvae_full_size_matches_digest():
    d = gu.load_npz('vqvae_train_full_digest.npz')
    img, _ = gu.synthetic_batch(128, 10, seed=73)
    img = img.cuda()
    m = _model(FULL, _full_state(d))
    tr, out = _step0(m, img)
    assert abs(float(out['loss']) - float(d['losses'][0])) < 1e-5
    hist = torch.bincount(out['code'].flatten().cpu(), minlength=512).numpy()
    assert np.array_equal(hist, d['hist0'])
    names = list(d['grad_names'])
    got = dict(m.named_parameters())
    floor = 1e-5 * float(d['grad_norms'].max())       # conv biases in front of a BatchNorm: zero up to rounding
    for k, ref in zip(names, d['grad_norms']):
        assert abs(float(got[k].grad.double().norm()) - ref) <= 1e-3 * ref + floor, k
    assert _rel(m.quantizer.cluster_size, d['cluster_size1']) < 1e-5
    assert _rel(m.quantizer.embedding, d['embedding1']) < 1e-5
    assert _rel(out['img'][:4, :, ::4, ::4], d['img0_sample']) < 1e-3
    from mcgen_amd.trainer import VQVAETrainer
    tr = VQVAETrainer(_model(FULL, _full_state(d)))
    tr.capture(img)
    losses = [float(tr.train_iteration(img)) for _ in range(2)]
    assert abs(losses[0] - d['losses'][0]) < 1e-5 and abs(losses[1] - d['losses'][1]) < 2e-3, (losses, d['losses'])


# ---- drivers ------------------------------------------------------------------------------------------------------
def _load_ck(path):
    sys.path.insert(0, os.path.join(ROOT, 'compat'))                       # the checkpoint pickles compat's Logger
    try:
        return torch.load(str(path), map_location='cpu', weights_only=False)
    finally:
        sys.path.remove(os.path.join(ROOT, 'compat'))


def _run(args, cwd):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_train_vqvae_driver_feeds_train_pixelcnn(tmp_path):
    drv = os.path.join(ROOT, 'compat')
    common = ['--data_name', 'CIFAR10', '--synthetic_size', '200', '--batch', '64', '--log_interval', '0.5']
    out = _run([os.path.join(drv, 'train_vqvae.py'), '--model_name', 'vqvae', '--control_name', 'None',
                '--num_epochs', '1'] + common, tmp_path)
    assert 'Experiment: 0_CIFAR10_label_vqvae' in out
    ck = tmp_path / 'output' / 'model' / '0_CIFAR10_label_vqvae_checkpoint.pt'
    assert ck.exists() and (tmp_path / 'output' / 'model' / '0_CIFAR10_label_vqvae_best.pt').exists()
    c = _load_ck(ck)
    assert c['epoch'] == 2 and {'cfg', 'model_dict', 'optimizer_dict', 'scheduler_dict', 'logger'} <= set(c)
    assert 'quantizer.embedding' in c['model_dict'] and 'quantizer.cluster_size' in c['model_dict']
    out = _run([os.path.join(drv, 'train_vqvae.py'), '--model_name', 'vqvae', '--control_name', 'None',
                '--num_epochs', '2', '--resume_mode', '1'] + common, tmp_path)
    assert 'Resume from 2' in out
    assert _load_ck(ck)['epoch'] == 3
    # 200 images at batch 64: the epoch ends in a batch of 8, which the captured PixelCNNTrainer runs eagerly
    out = _run([os.path.join(drv, 'train_pixelcnn.py'), '--model_name', 'mcpixelcnn', '--control_name', '0.5',
                '--num_epochs', '1'] + common + ['--log_interval', '0.2'], tmp_path)        # (0.2: every one of the 4 batches is logged)
    assert 'Not exists model tag: 0_CIFAR10_label_vqvae' not in out
    pk = _load_ck(tmp_path / 'output' / 'model' / '0_CIFAR10_label_mcpixelcnn_0.5_checkpoint.pt')
    assert pk['logger'].counter['train/Loss'] == 200                        # the logged train counter saw every image
