"""Short final batches on the HIP path: every epoch of a real dataset ends in a batch of another size than the captured one
(CIFAR-10: 390 x 128 + 80), down to a single sample.  For the eight single-network models (MCVAE, CVAE, MCGlow, CGlow,
MCPixelCNN, CPixelCNN, VQ-VAE, classifier), on their small fixtures' configuration, state and batch of B samples, fp32:

a. the engines at n = 1, 3 and B - 1 (the first n samples of the fixture's batch) against a float64 reference of the same
   step (short_batch_ref.py): loss and EVERY parameter's gradient through the autograd bridge; the two VAEs refuse n = 1 in
   training mode, as the reference's BatchNorm1d does, and leave everything as it was; bf16 at n = 3 tracks fp32;
b. a trainer captured at B, fed batches of B, B, 3, B, B - 1, B, against a twin that never captures: the short ones run the
   eager step at their own size, the graph and its statics stay as captured and replay correctly afterwards;
c. a batch of one sample does not broadcast into the captured statics;
d. refusals (inputs that disagree on N, another resolution; GraphedGANTrainer: any other batch size than the captured one)
   come before anything is copied or launched.

Bounds.  (a) per model the bound of its own gradient-vs-reference test at batch B (short_batch_ref.SPECS names the test each
comes from), or 4 x the float32-vs-float64 error of the reference alone where that is larger.  Measured by
test_short_batch_ref_cpu.py (reference only, no kernel involved), as a fraction of the model's own bound:

    model       n: loss error        worst gradient error / its bound at batch B
    mcvae       3: 4.3e-8  7: 3.9e-8     3: 0.037   7: 0.006
    cvae        3: 6.7e-8  7: 1.3e-8     3: 0.745   7: 0.079     (n = 3: encoder.blocks.0.bias 7.45e-8 against 1e-7)
    mcglow      1: 2.0e-7  3: 1.3e-6     1: 0.004   3: 0.010
    cglow       1: 3.8e-7  3: 6.5e-7     1: 0.005   3: 0.005
    mcpixelcnn  1: 1.3e-7  3: 1.4e-7  5: 6.2e-8     1: 0.020   3: 0.011   5: 0.007
    cpixelcnn   1: 4.9e-8  3: 7.1e-7  5: 4.3e-9     1: 0.275   3: 0.186   5: 0.146   (n = 1: two biases in front of a BatchNorm)
    vqvae       1: 4.2e-9  3: 5.5e-8  7: 3.3e-8     1: 0.039   3: 0.065   7: 0.040
    classifier  1: 2.7e-7  3: 3.9e-7 15: 3.3e-7     1: 0.079   3: 0.060  15: 0.076

so the bounds at batch B stand for every loss and for all but three gradients: cvae n = 3 encoder.blocks.0.bias
(3.0e-7 instead of 1e-7) and cpixelcnn n = 1 layers.0.horiz_resid.0.bias / output_conv.0.bias (1.1e-7 instead of 1e-7) --
biases in front of a BatchNorm, whose true gradient is zero and whose computed one is rounding residue.  The VQ-VAE and CGlow
references at n = 1 and B - 1 are digests (norm, sum, max |g| per parameter): an elementwise error below the bound moves
the norm by at most sqrt(numel) and the sum by at most numel times it (short_batch_ref.check_gradient).
(b, c, d) graph against eager: each model's own graph-vs-eager bound (GRAPH below names the tests).

(c) A batch of B copies of one sample has the batch statistics, the mean loss and the gradients of that one sample
(test_short_batch_ref_cpu.py::test_a_batch_of_copies_has_the_loss_of_one_sample), so the LOSS cannot show a broadcast.  What
shows it: the statics (overwritten by the copies), and the state a step leaves -- the running variances (unbiased:
m / (m - 1)) and the VQ-VAE's cluster counts; those are what the test pins.
"""
import numpy as np
import pytest
import torch

import golden_util as gu
import short_batch_ref as S

pytestmark = pytest.mark.gpu

# graph-vs-eager bounds, (absolute, relative to max |reference|) for the loss and for every state tensor; (0, 0) is bitwise:
# test_mcvae_gpu.py::test_replay_follows_a_learning_rate_change_without_recapture (1e-6 (1 + |x|));
# test_cvae_gpu.py / test_cpixelcnn_gpu.py::test_graphed_step_equals_eager_and_bf16_tracks_fp32 (bitwise);
# test_mcglow_gpu.py::test_mcglow_graphed_trainer_tracks_eager, test_cglow_gpu.py::test_cglow_graphed_trainer_tracks_eager,
# test_mcpixelcnn_gpu.py::test_pixelcnn_train_steps_vs_reference (losses within 1e-5);
# test_vqvae_train_gpu.py::test_vqvae_graphed_trainer_equals_eager_and_bridge_gradients (loss 1e-6, state 1e-6 of its max);
# test_classifier_train_gpu.py::test_graphed_trainer_equals_eager_bitwise
GRAPH = {'mcvae': ((1e-6, 1e-6), (1e-6, 1e-6)), 'cvae': ((0, 0), (0, 0)), 'mcglow': ((1e-5, 0), (1e-5, 0)),
         'cglow': ((1e-5, 0), (1e-5, 0)), 'mcpixelcnn': ((1e-5, 0), None), 'cpixelcnn': ((0, 0), (0, 0)),
         'vqvae': ((1e-6, 0), (0, 1e-6)), 'classifier': ((0, 0), (0, 0))}
# MCPixelCNN's state: its code embedding's gradient is an index_add_ whose float atomics add in an order that varies from run
# to run, so from the second step on two runs differ in rounding, and Adam turns the rounding-residue gradients
# of the biases in front of a BatchNorm into steps of up to lr of either sign: 2 lr per step, the bound of
# test_mcpixelcnn_gpu.py::test_pixelcnn_train_steps_vs_reference.  The losses keep that test's 1e-5.
STATE_PER_STEP = {'mcpixelcnn': 2 * 3e-4}
ONE_OK = [m for m in S.MODELS if S.SPECS[m].one_ok]


def _sync():
    """Wait for the launches; a device-side fault ends the whole session -- nothing more is launched on a faulted GPU."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault, stopping the session: {e}', returncode=3)


def _build(name, dtype=torch.float32):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name=name, data_name='COIL100' if name == 'classifier' else 'CIFAR10', device='cuda', controller_rate=0.5,
               classes_size={'mcglow': 12, 'cglow': 12, 'classifier': 100}.get(name, 10), compute_dtype='float32',
               data_shape=[1, 32, 32] if name in ('mcglow', 'cglow') else [3, 32, 32])
    cfg['vae'] = {'hidden_size': [8, 16, 32], 'latent_size': 16, 'num_res_block': 2, 'embedding_size': 32}
    cfg['glow'] = {'hidden_size': 32, 'K': 2, 'L': 3, 'affine': True, 'conv_lu': True}
    cfg['pixelcnn'] = {'num_layer': 4, 'hidden_size': 16, 'num_embedding': 32}
    cfg['vqvae'] = {'hidden_size': [16, 16], 'num_res_block': 2, 'embedding_size': 8, 'num_embedding': 64, 'vq_commit': 0.25}
    cfg['classifier'] = {'hidden_size': [8, 16, 32, 64]}
    np.random.seed(0)
    m = getattr(models, name)()
    m.load_state_dict(S.state(name), strict=True)
    m = m.cuda().set_compute_dtype(dtype)
    m.train(True)
    return m


def _trainer(name, m):
    from mcgen_amd import trainer as T
    if name == 'classifier':
        return T.ClassifierTrainer(m, lr=1e-2)
    cls = {'mcvae': T.VAETrainer, 'cvae': T.VAETrainer, 'mcglow': T.GlowTrainer, 'cglow': T.GlowTrainer,
           'mcpixelcnn': T.PixelCNNTrainer, 'cpixelcnn': T.PixelCNNTrainer, 'vqvae': T.VQVAETrainer}[name]
    return cls(m)


def _cuda(b):
    return {k: v.cuda() for k, v in b.items()}


def _args(b):
    """The input dict in train_iteration's order: img[, label[, eps | noise]]."""
    return [b[k] for k in ('img', 'label', 'eps', 'noise') if k in b]


def _step(tr, b):
    loss = tr.train_iteration(*_args(b))
    _sync()
    return loss.detach().clone()


def _close(a, b, bound, what):
    ab, rel = bound
    a, b = a.detach(), b.detach()
    if not a.is_floating_point() or (ab == 0 and rel == 0):
        assert torch.equal(a, b), what
        return
    err, tol = float((a.double() - b.double()).abs().max()), ab + rel * float(b.double().abs().max())
    assert err <= tol, (what, err, tol)


def _same_state(name, ta, te, what):
    sa, se = ta.model.state_dict(), te.model.state_dict()
    assert list(sa) == list(se)
    assert int(ta.opt.step_count) == int(te.opt.step_count), what
    bound = GRAPH[name][1]
    if name in STATE_PER_STEP:
        bound = (STATE_PER_STEP[name] * int(te.opt.step_count), 0)
    for k in se:
        _close(sa[k], se[k], bound, (name, what, k))


def _frozen(tr):
    """Bit copies of everything a step may write: parameters, buffers, gradients, optimizer state, captured statics."""
    ts = dict(tr.model.state_dict())
    ts.update({f'grad/{k}': p.grad for k, p in tr.model.named_parameters() if p.grad is not None})
    ts.update({f'opt/{i}': t for i, t in enumerate(tr.opt.state_tensors())})
    ts.update({f'static/{i}': t for i, t in enumerate(getattr(tr, 'statics', ()))})
    ts['gflat'] = tr.gflat
    return ts, {k: v.detach().clone() for k, v in ts.items()}


def _unchanged(snap, what):
    live, kept = snap
    _sync()
    for k, v in live.items():
        assert torch.equal(v.detach(), kept[k]), (what, k)


# ---- a. the engines at short N against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name,n', [(m, n) for m in S.MODELS for n in S.sizes(m) if n > 1 or S.SPECS[m].one_ok])
def test_engine_at_short_batch_matches_float64(name, n):
    m = _build(name)
    out = m(_cuda(S.batch(name, n)))
    out['loss'].backward()
    _sync()
    ref = S.reference(name, n)
    bloss, _ = S.bounds(name, n)
    eloss = abs(float(out['loss'].detach()) - ref.loss)
    named = dict(m.named_parameters())
    checked, worst = 0, (0.0, None)
    for k, p in named.items():
        err, bound = S.check_gradient(name, n, k, p.grad)
        if bound > 0:
            worst = max(worst, (err / bound, k))
        checked += 1
    print(f'{name} n={n}: loss {float(out["loss"].detach()):.8f} ref {ref.loss:.8f} err {eloss:.2e} (bound {bloss:.1e}); '
          f'worst gradient error / bound {worst}')
    assert eloss < bloss, (name, n, eloss, bloss)
    assert checked == len(dict(m.named_parameters())) and checked >= 18


@pytest.mark.parametrize('name', ['mcvae', 'cvae'])
def test_vae_refuses_one_sample_in_training_mode(name):
    """The reference raises there (nn.BatchNorm1d over one value per channel); ours raises ValueError before any launch, through
    the bridge and through the trainer, and normalises nothing: parameters, buffers, gradients and optimizer state stay bit
    for bit.  Evaluation mode at N = 1 stays legal."""
    m = _build(name)
    tr = _trainer(name, m)
    _step(tr, _cuda(S.batch(name, 3)))                                      # (so that gradients and moments are not all zero)
    snap = _frozen(tr)
    one = _cuda(S.batch(name, 1))
    with pytest.raises(ValueError, match='Not valid batch'):
        m(one)
    with pytest.raises(ValueError, match='Not valid batch'):
        tr.train_iteration(*_args(one))
    with pytest.raises(ValueError, match='Not valid batch'):
        tr.train_iteration(one['img'], one['label'])                        # (noise drawn by the trainer)
    _unchanged(snap, name)
    tr.capture(*_args(_cuda(S.batch(name)))[:2])
    snap = _frozen(tr)
    with pytest.raises(ValueError, match='Not valid batch'):
        tr.train_iteration(*_args(one))
    _unchanged(snap, name + ' captured')
    m.train(False)
    with torch.no_grad():
        ev = m(one)
    _sync()
    assert np.isfinite(float(ev['loss'])) and ev['img'].shape[0] == 1


@pytest.mark.parametrize('name', S.MODELS)
def test_bf16_tracks_fp32_at_three_samples(name):
    b = _cuda(S.batch(name, 3))
    with torch.no_grad():
        l32 = float(_build(name)(b)['loss'])
        l16 = float(_build(name, torch.bfloat16)(b)['loss'])
    _sync()
    bound = S.SPECS[name].bf16_loss * (abs(l32) if name == 'classifier' else 1.0)
    print(f'{name}: bf16 {l16:.6f} fp32 {l32:.6f} bound {bound:.1e}')
    assert abs(l32 - S.reference(name, 3).loss) < S.bounds(name, 3)[0]
    assert abs(l16 - l32) < bound, (name, l16, l32)


# ---- b. a captured trainer takes short batches ------------------------------------------------------------------------------
def _twins(name):
    ta, te = _trainer(name, _build(name)), _trainer(name, _build(name))
    full = _cuda(S.batch(name))
    before = {k: v.detach().clone() for k, v in ta.model.state_dict().items()}
    ta.capture(*_args(full)[:1 if name == 'vqvae' else 2])
    _sync()
    for k, v in ta.model.state_dict().items():                              # capture does not advance training
        assert torch.equal(v, before[k]), k
    return ta, te


@pytest.mark.parametrize('name', S.MODELS)
def test_captured_trainer_takes_short_batches(name):
    B = S.SPECS[name].B
    ta, te = _twins(name)
    shape = tuple(ta.statics[0].shape)
    assert shape[0] == B
    for i, n in enumerate([B, B, 3, B, B - 1, B]):
        b = _cuda(S.batch(name, n))
        statics = [t.detach().clone() for t in ta.statics]
        la, le = _step(ta, b), _step(te, b)
        _close(la, le, GRAPH[name][0], (name, i, n, float(la), float(le)))
        assert tuple(ta.statics[0].shape) == shape
        if n != B:                                                          # the eager step left the captured inputs alone
            assert all(torch.equal(s, t) for s, t in zip(statics, ta.statics)), (name, i, n)
        else:
            assert torch.equal(ta.statics[0], b['img'])
        assert int(ta.opt.step_count) == i + 1 and int(te.opt.step_count) == i + 1
    _same_state(name, ta, te, 'after the sequence')
    if len(_args(b)) == 3:                          # a short batch without injected noise draws it at the batch's own size
        short = _cuda(S.batch(name, 3))
        assert np.isfinite(float(_step(ta, {k: short[k] for k in ('img', 'label')})))
        assert tuple(ta.statics[2].shape)[0] == B


# ---- c. one sample does not broadcast ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ONE_OK)
def test_one_sample_does_not_broadcast(name):
    B = S.SPECS[name].B
    ta, te = _twins(name)
    one = _cuda(S.batch(name, 1))
    statics = [t.detach().clone() for t in ta.statics]
    la, le = _step(ta, one), _step(te, one)
    _close(la, le, GRAPH[name][0], (name, float(la), float(le)))
    assert all(torch.equal(s, t) for s, t in zip(statics, ta.statics)), name      # copy_ would have filled them with B copies
    _same_state(name, ta, te, 'after one sample')
    # a step on B copies of that sample (what the broadcast trained on) leaves another state, though not another loss
    tc = _trainer(name, _build(name))
    lc = _step(tc, {k: v.expand(B, *v.shape[1:]).contiguous() for k, v in one.items()})
    print(f'{name}: one sample {float(la):.8f}, {B} copies {float(lc):.8f}')
    sa, sc = ta.model.state_dict(), tc.model.state_dict()
    moved = [k for k in sa if k.endswith(('running_var', 'cluster_size')) and not torch.allclose(sa[k], sc[k], rtol=1e-4, atol=0)]
    has = [k for k in sa if k.endswith(('running_var', 'cluster_size'))]
    # (m / (m - 1) with m = H W against B H W: 1.3e-3 of a unit variance at 8 x 8, times the momentum 0.1; some stage is small)
    assert bool(moved) == bool(has), (name, has)
    full = _cuda(S.batch(name))
    _close(_step(ta, full), _step(te, full), GRAPH[name][0], (name, 'the replay after it'))
    _same_state(name, ta, te, 'after the replay')


# ---- d. refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', S.MODELS)
def test_flat_trainers_refuse_mismatched_batches(name):
    ta, tt = _trainer(name, _build(name)), _trainer(name, _build(name))
    full = _cuda(S.batch(name))
    for t in (ta, tt):
        t.capture(*_args(full)[:1 if name == 'vqvae' else 2])
    _step(ta, full), _step(tt, full)
    snap = _frozen(ta)
    bad = []
    short = _cuda(S.batch(name, 3))
    if 'label' in full:
        bad.append(dict(short, label=full['label'][:2]))                    # inputs disagree on N
        bad.append(dict(full, label=full['label'][:1]))                     # a label copy_ would broadcast
    half = {k: (v[..., ::2, ::2].contiguous() if k in ('img', 'noise') else v) for k, v in short.items()}
    bad.append(half)                                                        # another resolution at a short size
    bad.append({k: (v[..., ::2, ::2].contiguous() if k in ('img', 'noise') else v) for k, v in full.items()})
    if len(_args(full)) == 3:
        bad.append(dict(short, **{k: full[k] for k in ('eps', 'noise') if k in full}))     # noise of another N than the batch
    for b in bad:
        with pytest.raises(ValueError, match='Not valid batch'):
            ta.train_iteration(*_args(b))
        _unchanged(snap, (name, {k: tuple(v.shape) for k, v in b.items()}))
    la, lt = _step(ta, full), _step(tt, full)
    _close(la, lt, GRAPH[name][0], (name, float(la), float(lt)))
    _same_state(name, ta, tt, 'after the refusals')


def _gan(name):
    from mcgen_amd import models
    from mcgen_amd.config import cfg, process_control
    d = gu.load_npz(f'{name}_small.npz')
    cfg['data_name'], cfg['model_name'], cfg['device'] = 'CIFAR10', name, 'cuda'
    cfg.pop('classes_size', None)
    process_control()
    cfg['classes_size'] = 10
    cfg['gan']['generator_hidden_size'], cfg['gan']['discriminator_hidden_size'] = [32] * 4, [16] * 4
    if name == 'mcgan':
        sd = gu.state_from_npz(d)
    else:
        import cglow_ref
        sd = gu.procedural_state_generic(cglow_ref.layout(d), seed=int(d['sd_seed']))
    m = getattr(models, name)()
    m.load_state_dict(sd, strict=True)
    return d, m.cuda().set_compute_dtype(torch.float32)


@pytest.mark.parametrize('name', ['mcgan', 'cgan'])
def test_graphed_gan_trainer_refuses_another_batch_size(name):
    """The paired and grouped passes are sized at capture: a batch of B - 1 or of one sample raises ValueError before s_img /
    s_label are touched (copy_ would raise late for B - 1 and broadcast silently for 1).  The next replay equals a twin's, to
    the bound of test_gan_replay_forms_gpu.py (1e-6 + 1e-5 max |v|) for MCGAN and bit for bit for CGAN (test_cgan_gpu.py::
    test_graphed_matches_eager)."""
    from mcgen_amd.trainer import GraphedGANTrainer
    bound = (1e-6, 1e-5) if name == 'mcgan' else (0, 0)
    trainers = []
    for _ in range(2):
        d, m = _gan(name)
        tr = GraphedGANTrainer(m, 10)
        img, lab = torch.from_numpy(d['img']).cuda(), torch.from_numpy(d['label']).cuda()
        tr.capture(img, lab)
        trainers.append(tr)
    ta, tt = trainers
    zs = [torch.from_numpy(z).cuda() for z in d['z'][:6]]
    B = img.shape[0]
    live = ta._state_tensors() + [ta.s_img, ta.s_label, ta.s_zall]
    _sync()
    kept = [t.detach().clone() for t in live]
    for n in (B - 1, 1):
        for z in (None, [v[:n] for v in zs]):
            with pytest.raises(ValueError, match='Not valid batch'):
                ta.train_iteration(img[:n], lab[:n], z)
        with pytest.raises(ValueError, match='Not valid batch'):
            ta.train_iteration(img, lab[:n], zs)
        _sync()
        for i, (t, k) in enumerate(zip(live, kept)):
            assert torch.equal(t, k), (name, n, i)
    la = [v.detach().clone() for v in ta.train_iteration(img, lab, zs)]
    lt = [v.detach().clone() for v in tt.train_iteration(img, lab, zs)]
    _sync()
    for a, b in zip(la, lt):
        _close(a, b, bound, (name, float(a), float(b)))
    sa, st = ta.model.state_dict(), tt.model.state_dict()
    for k in st:
        _close(sa[k], st[k], bound, (name, k))
    assert int(ta.opt_d.step_count) == int(tt.opt_d.step_count) == 5 and int(ta.opt_g.step_count) == int(tt.opt_g.step_count) == 1
