"""GPU parity of the CPixelCNN kernels (csrc/cpixelcnn_ops.hip) against fp64 torch restatements, and of the model
(models/cpixelcnn.py on cpixelcnn_engine.py) against the reference-generated fixtures tests/golden/cpixelcnn_*.npz:
forward, gradients, train steps, graphed steps, bf16, incremental sampling and the driver pipeline."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
from cpixelcnn_ref import ref_module as _ref_module
from test_cpixelcnn_cpu import layout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _gate_ref(s, e, label, gamma, beta, g, train=True, rm=None, rv=None):
    """fp64 restatement of GatedActivation(s + e[label]) (cpixelcnn.py:14-18, 52, 56) on NHWC s; returns
    (out, ds, dgamma, dbeta, de, mean, var) with de the gradient of the embedding table."""
    s = s.double().clone().requires_grad_(True)
    e = e.double().clone().requires_grad_(True)
    gamma = gamma.double().clone().requires_grad_(True)
    beta = beta.double().clone().requires_grad_(True)
    c = s.shape[-1] // 2
    x = s + e[label][:, None, None, :]
    a, b = x[..., :c], x[..., c:]
    if train:
        mean, var = a.mean((0, 1, 2)), a.var((0, 1, 2), unbiased=False)
    else:
        mean, var = rm.double(), rv.double()
    z = (a - mean) / torch.sqrt(var + 1e-5) * gamma + beta
    out = torch.relu(z) * torch.sigmoid(b)
    (out * g.double()).sum().backward()
    return out.detach(), s.grad, gamma.grad, beta.grad, e.grad, mean.detach(), var.detach()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('modes,c', [(10, 16), (1623, 128)])
def test_conditional_gate_kernels(dtype, modes, c):
    from mcgen_amd import ops
    g = torch.Generator().manual_seed(modes + c)
    n, h = 12, 8
    # the per-sample rows dominate the variance: statistics rebuilt from whole-batch sums of s would cancel here
    s = (0.1 * torch.randn(n, h, h, 2 * c, generator=g)).to(dtype).float()
    table = 4.0 * torch.randn(modes, 2 * c, generator=g) + 3.0
    label = torch.tensor([0, 5, 5, modes - 1, 2, 5, 0, 7, modes - 1, 3, 3, 1])                  # repeats; most modes absent
    gamma, beta = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    go = torch.randn(n, h, h, c, generator=g).to(dtype).float()
    out_r, ds_r, dg_r, db_r, de_r, mean_r, var_r = _gate_ref(s, table, label, gamma, beta, go)
    sd, td, ld = s.to(dtype).cuda(), table.cuda(), label.cuda()
    f32 = dtype == torch.float32
    # statistics: one launch for two gates (the second on a different input), finalized by the unchanged bn_finalize_batch
    s2 = s.flip(0).contiguous()
    parts = ops.cpx_gate_stats([(sd, td, ld), (s2.to(dtype).cuda(), td, ld)])
    count = n * h * h
    rm, rv = torch.zeros(c, device='cuda'), torch.ones(c, device='cuda')
    (sc, sh, mean, rstd), = ops.bn_finalize_batch([(parts[0], count, gamma.cuda(), beta.cuda(), rm, rv, 0.1, 1e-5)])
    assert _rel(mean, mean_r) < 1e-6 and _rel(1 / rstd ** 2 - 1e-5, var_r) < 1e-5
    assert _rel(rm, 0.1 * mean_r) < 1e-6 and _rel(rv, 0.9 + 0.1 * var_r * count / (count - 1)) < 1e-5
    a2 = s2 + table[label.flip(0)][:, None, None, :]
    p2 = parts[1].double().sum(0)
    assert _rel(p2[0] / count, a2[..., :c].double().mean((0, 1, 2))) < 1e-6
    # forward
    out, out2 = ops.cpx_gated_fwd([(sd, td, ld, sc, sh), (sd, td, ld, sc, sh)])
    assert torch.equal(out, out2)
    assert _rel(out.float(), out_r) < (1e-5 if f32 else 1e-2)
    # backward: input gradient, BatchNorm parameter gradients, per-image sums, embedding gradient
    dg, db = torch.zeros(c, device='cuda'), torch.zeros(c, device='cuda')
    ds, dsum = ops.cpx_gated_bwd(sd, td, ld, sc, sh, mean, rstd, go.to(dtype).cuda(), dg, db)
    assert _rel(ds.float(), ds_r) < (5e-5 if f32 else 2e-2)
    assert _rel(dg, dg_r) < (5e-5 if f32 else 1e-2) and _rel(db, db_r) < (5e-5 if f32 else 1e-2)
    assert _rel(dsum, ds_r.sum((1, 2))) < (5e-5 if f32 else 1e-2)
    de = torch.full((modes, 2 * c), float('nan'), device='cuda')
    ops.cpx_embed_bwd(None, dsum, ld, de)
    assert _rel(de, de_r) < (5e-5 if f32 else 1e-2)
    absent = torch.ones(modes, dtype=torch.bool)
    absent[label] = False
    assert float(de[absent.cuda()].abs().max()) == 0.0
    # two gates: dE = sum of both per-image sums, in ascending n (bit-identical reruns)
    de2 = torch.empty_like(de)
    ops.cpx_embed_bwd(dsum, dsum, ld, de2)
    assert _rel(de2, 2 * de_r) < (5e-5 if f32 else 1e-2)
    de3 = torch.empty_like(de)
    ops.cpx_embed_bwd(dsum, dsum, ld, de3)
    assert torch.equal(de2, de3)
    # the sampler's row gather
    tables = torch.stack([table, -table]).cuda()
    rows = ops.cpx_gather_rows(tables, ld)
    assert torch.equal(rows.cpu(), torch.stack([table[label], -table[label]]))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_code_embedding_gradient_kernel(dtype):
    """dE[k] = sum of dx over the pixels whose code is k, in ascending pixel order: bit-identical reruns, absent codes 0,
    a code outside [0, K) adds nothing."""
    from mcgen_amd import ops
    g = torch.Generator().manual_seed(5)
    n, h, c, k = 128, 8, 128, 512
    codes = torch.randint(0, k - 40, (n, h, h), generator=g)                  # the last 40 codes are absent
    codes[0, 0, :3] = torch.tensor([-1, k, 10 ** 9])
    dx = torch.randn(n, h, h, c, generator=g).to(dtype).float()
    keep = (codes >= 0) & (codes < k)
    ref = torch.zeros(k, c, dtype=torch.float64).index_add_(0, codes[keep], dx[keep].double())
    de = torch.full((k, c), float('nan'), device='cuda')
    ops.cpx_code_embed_bwd(dx.to(dtype).cuda(), codes.cuda(), de)
    assert _rel(de, ref) < 1e-6
    assert float(de[k - 40:].abs().max()) == 0.0
    de2 = torch.empty_like(de)
    ops.cpx_code_embed_bwd(dx.to(dtype).cuda(), codes.cuda(), de2)
    assert torch.equal(de, de2)


def test_out_of_range_labels_stay_inside_the_table():
    """Labels cannot be checked on the host during graph replay: gathers clamp, the embedding gradient skips them."""
    from mcgen_amd import ops
    c, modes = 16, 5
    s = torch.randn(2, 4, 4, 2 * c).cuda()
    table = torch.randn(modes, 2 * c).cuda()
    bad = torch.tensor([-3, 99]).cuda()
    clamped = torch.tensor([0, modes - 1]).cuda()
    sc, sh = torch.ones(c).cuda(), torch.zeros(c).cuda()
    assert torch.equal(ops.cpx_gated_fwd([(s, table, bad, sc, sh)])[0], ops.cpx_gated_fwd([(s, table, clamped, sc, sh)])[0])
    assert torch.equal(ops.cpx_gate_stats([(s, table, bad)])[0], ops.cpx_gate_stats([(s, table, clamped)])[0])
    de = torch.full((modes, 2 * c), 7.0).cuda()
    ops.cpx_embed_bwd(None, torch.ones(2, 2 * c).cuda(), bad, de)
    assert float(de.abs().max()) == 0.0
    assert torch.equal(ops.cpx_gather_rows(table[None].contiguous(), bad), ops.cpx_gather_rows(table[None].contiguous(), clamped))


def _init_state(d):
    return gu.procedural_state_generic(layout(d), seed=int(d['sd_seed']))


def _final_state(d):
    out = {}
    for k, v in _init_state(d).items():
        out[k] = torch.from_numpy(np.array(d['sd_final_int/' + k])) if 'sd_final_int/' + k in d else \
            v + torch.from_numpy(d['sd_delta/' + k])
    return out


def _model(sd, classes, hidden=16, layers=4, codes=32, dtype=torch.float32):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name='cpixelcnn', device='cuda', classes_size=classes, compute_dtype='float32')
    cfg['pixelcnn'] = {'num_layer': layers, 'hidden_size': hidden, 'num_embedding': codes}
    m = models.cpixelcnn()
    m.load_state_dict(sd)
    return m.cuda().set_compute_dtype(dtype)


@pytest.mark.parametrize('fixture,classes', [('cpixelcnn_small.npz', 10), ('cpixelcnn_omniglot_small.npz', 1623)])
def test_cpixelcnn_vs_reference(fixture, classes):
    from mcgen_amd.trainer import PixelCNNTrainer
    d = gu.load_npz(fixture)
    codes, lab = torch.from_numpy(d['codes']).cuda(), torch.from_numpy(d['label']).cuda()
    m = _model(_init_state(d), classes)
    m.train(True)
    with torch.no_grad():
        out = m({'img': codes, 'label': lab})
    assert abs(float(out['loss']) - float(d['losses'][0])) < 1e-4
    assert _rel(out['logits'], d['logits0']) < 2e-4
    assert float(m.layers[0].vert_stack.weight[:, :, -1].abs().max()) == 0.0
    assert int(m.layers[1].gate_v.bn.num_batches_tracked) == 1
    # three train_pixelcnn.py steps (Adam, clip 1) and the state they leave
    m = _model(_init_state(d), classes)
    tr = PixelCNNTrainer(m)
    losses = [float(tr.train_iteration(codes, lab)) for _ in range(3)]
    assert abs(losses[0] - d['losses'][0]) < 1e-4, (losses, d['losses'])
    assert max(abs(a - b) for a, b in zip(losses, d['losses'])) < 3e-3, (losses, d['losses'])
    sd = m.state_dict()
    if 'sd_delta/embedding.weight' in d:
        for k, v in _final_state(d).items():
            if v.is_floating_point():
                assert float((sd[k].cpu() - v).abs().max()) < 2e-3, k
            else:
                assert torch.equal(sd[k].cpu(), v), k
        # the embedding rows of absent modes never move; the present ones do
        e0, e1 = _init_state(d)['layers.1.class_cond_embedding.weight'], sd['layers.1.class_cond_embedding.weight'].cpu()
        present = torch.zeros(classes, dtype=torch.bool)
        present[torch.from_numpy(d['label'])] = True
        assert torch.equal(e0[~present], e1[~present]) and float((e0[present] - e1[present]).abs().min()) > 0
    else:
        for k, v in sd.items():
            if not v.is_floating_point():
                continue
            got, ref = gu.checksum(v.float().cpu()), d['digest/' + k]
            if k.endswith(('horiz_resid.0.bias', 'output_conv.0.bias')):
                # a bias in front of a BatchNorm has an exactly-zero gradient: Adam turns rounding residue into steps of up
                # to lr, different here and there -- only that bound holds (3 steps of 3e-4 per element)
                assert np.abs(got - ref).max() < 2 * 3 * 3e-4 * v.numel(), (k, got, ref)
                continue
            assert np.abs(got - ref).max() < 2e-3 * max(float(ref[1]), 1.0), (k, got, ref)
    # eval mode on the trained reference state
    full = 'sd_delta/embedding.weight' in d                  # else: evaluate the state trained here (digests only stored)
    m = _model(_final_state(d) if full else sd, classes)
    m.train(False)
    with torch.no_grad():
        out = m({'img': codes, 'label': lab})
    assert _rel(out['logits'], d['logits_eval']) < (5e-4 if full else 5e-3)


def test_gradients_vs_reference_autograd():
    """Step-0 gradients of every parameter (through the autograd bridge) against an fp64 reference restated in torch on the
    CPU with the reference's own module classes."""
    d = gu.load_npz('cpixelcnn_small.npz')
    sd = _init_state(d)
    codes, lab = torch.from_numpy(d['codes']), torch.from_numpy(d['label'])
    m = _model(sd, 10)
    m.train(True)
    out = m({'img': codes.cuda(), 'label': lab.cuda()})
    out['loss'].backward()
    ref = _ref_module(sd, 10)
    rout = ref(codes, lab)
    rout.backward()
    named = dict(ref.named_parameters())
    for k, p in m.named_parameters():
        rg = named[k].grad
        if rg is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        err = float((p.grad.double().cpu() - rg).abs().max())
        assert err < 5e-4 * float(rg.abs().max()) + 1e-7, (k, err)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_cpixelcnn_full_size_digest(dtype):
    """configs[4] shapes at batch 128 (6,406,016 parameters) against cpixelcnn_full_digest.npz: first loss and logits
    digest, every parameter gradient digest of that step, two train_pixelcnn.py steps."""
    from mcgen_amd.trainer import PixelCNNTrainer
    d = gu.load_npz('cpixelcnn_full_digest.npz')
    f32 = dtype == torch.float32

    def build():
        return _model(_init_state(d), 10, 128, 15, 512, dtype)
    m = build()
    assert sum(p.numel() for p in m.parameters()) == 6406016
    codes, lab = torch.from_numpy(d['codes']).cuda(), torch.from_numpy(d['label']).cuda()
    m.train(True)
    out = m({'img': codes, 'label': lab})
    assert abs(float(out['loss']) - float(d['losses'][0])) < (2e-4 if f32 else 5e-2)
    got, ref = gu.checksum(out['logits'].float().detach().cpu()), d['logits0_digest']
    assert np.abs(got - ref).max() < (1e-3 if f32 else 3e-2) * ref[1], (got, ref)
    out['loss'].backward()
    named = dict(m.named_parameters())
    assert set(map(str, d['grad_keys'])) | set(map(str, d['nograd_keys'])) == set(named)
    assert 'layers.14.gate_v.bn.weight' in set(map(str, d['nograd_keys']))
    worst = (0.0, None)
    for k in map(str, d['grad_keys']):
        gp = named[k].grad
        assert gp is not None, k
        got, ref = gu.checksum(gp.float().cpu()), d['grad0_digest/' + k]
        numel = gp.numel()
        if float(ref[1]) / numel < 1e-7:                     # exactly zero in exact arithmetic (a bias before a BatchNorm)
            assert float(got[1]) / numel < (1e-6 if f32 else 1e-4), (k, got, ref)
            continue
        err = float(np.abs(got - ref).max()) / float(ref[1])
        worst = max(worst, (err, k))
        assert err < (2e-3 if f32 else 1e-1), (k, got, ref)
    print('worst gradient digest error (relative to sum |g|):', worst)
    for k in map(str, d['nograd_keys']):
        assert named[k].grad is None or float(named[k].grad.abs().max()) == 0.0, k
    tr = PixelCNNTrainer(build())
    losses = [float(tr.train_iteration(codes, lab)) for _ in range(2)]
    print('train losses', losses, 'reference', d['losses'])
    assert abs(losses[0] - d['losses'][0]) < (2e-4 if f32 else 5e-2)
    assert abs(losses[1] - d['losses'][1]) < (5e-3 if f32 else 1.5e-1)


def test_graphed_step_equals_eager_and_bf16_tracks_fp32():
    from mcgen_amd.trainer import PixelCNNTrainer
    d = gu.load_npz('cpixelcnn_omniglot_small.npz')
    codes, lab = torch.from_numpy(d['codes']).cuda(), torch.from_numpy(d['label']).cuda()
    eager = PixelCNNTrainer(_model(_init_state(d), 1623))
    le = [float(eager.train_iteration(codes, lab)) for _ in range(3)]
    graphed = PixelCNNTrainer(_model(_init_state(d), 1623))
    graphed.capture(codes, lab)
    lg = [float(graphed.train_iteration(codes, lab)) for _ in range(3)]
    assert le == lg, (le, lg)
    # every reduction of the step runs in a fixed order (no float atomics): the replayed graph leaves the eager step's state
    # bit for bit -- even the biases in front of a BatchNorm, whose rounding-residue gradients Adam turns into full steps
    se, sg = eager.model.state_dict(), graphed.model.state_dict()
    for k in se:
        assert torch.equal(se[k], sg[k]), k
    bf = PixelCNNTrainer(_model(_init_state(d), 1623, dtype=torch.bfloat16))
    lb = [float(bf.train_iteration(codes, lab)) for _ in range(3)]
    assert max(abs(a - b) for a, b in zip(lb, le)) < 5e-2, (lb, le)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_sample_matches_eval_forward(dtype):
    """The incremental sampler's logits at every position equal one eval-mode forward of the drawn map."""
    d = gu.load_npz('cpixelcnn_small.npz')
    m = _model(_final_state(d), 10, dtype=dtype)
    m.train(False)
    lab = torch.tensor([0, 3, 3, 9, 5, 1, 2, 2, 7, 4, 8, 6, 0, 9, 3, 1, 5]).cuda()            # 17: two sample tiles
    x, logits = m.sample(lab, return_logits=True)
    with torch.no_grad():
        ref = m({'img': x, 'label': lab})['logits']
    assert _rel(logits, ref.float()) < (2e-5 if dtype == torch.float32 else 3e-2)
    assert int(x.min()) >= 0 and int(x.max()) < 32


def test_greedy_sample_equals_reference_greedy_decode():
    d = gu.load_npz('cpixelcnn_small.npz')
    m = _model(_final_state(d), 10)
    m.train(False)
    lab = torch.from_numpy(d['label']).cuda()
    x = m.sample(lab, greedy=True)
    assert torch.equal(x.cpu(), torch.from_numpy(d['greedy']))
    y = m.generate(lab, sampler=lambda p: p.argmax(-1))
    assert torch.equal(y.cpu(), torch.from_numpy(d['greedy']))


def test_sample_contract():
    d = gu.load_npz('cpixelcnn_small.npz')
    m = _model(_final_state(d), 10)
    lab = torch.tensor([1, 2]).cuda()
    with pytest.raises(ValueError):
        m.sample(lab)                                                   # training mode
    m.train(False)
    with pytest.raises(ValueError):
        m.sample(lab.int())
    with pytest.raises(ValueError):
        m.sample(torch.tensor([1, 10]).cuda())
    u = torch.rand(64, 2, generator=torch.Generator().manual_seed(3)).cuda()
    a = m.sample(lab, uniform=u)
    b = m.sample(lab, uniform=u)
    assert torch.equal(a, b) and a.shape == (2, 8, 8)


def _run(args, cwd):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_driver_pipeline(tmp_path):
    drv = os.path.join(ROOT, 'compat')
    common = ['--data_name', 'CIFAR10', '--log_interval', '0.5']
    _run([os.path.join(drv, 'train_vqvae.py'), '--model_name', 'vqvae', '--control_name', 'None', '--num_epochs', '1',
          '--synthetic_size', '200', '--batch', '64'] + common, tmp_path)
    _run([os.path.join(drv, 'train_pixelcnn.py'), '--model_name', 'cpixelcnn', '--control_name', 'None', '--num_epochs', '1',
          '--synthetic_size', '192', '--batch', '64'] + common, tmp_path)
    tag = '0_CIFAR10_label_cpixelcnn'
    assert (tmp_path / 'output' / 'model' / f'{tag}_best.pt').exists()
    out = _run([os.path.join(drv, 'generate.py'), '--model_name', 'cpixelcnn', '--control_name', 'None', '--save_npy', 'True',
                '--generate_per_mode', '2', '--synthetic_size', '192'] + common, tmp_path)
    assert f'Experiment: {tag}' in out and 'Not exists model tag' not in out
    a = np.load(tmp_path / 'output' / 'npy' / f'generated_{tag}.npy')
    assert a.shape == (20, 3, 32, 32) and np.isfinite(a).all()
