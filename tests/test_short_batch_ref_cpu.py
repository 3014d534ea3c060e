"""CPU side of the short-batch tests (no GPU): the float64 references of test_short_batch_gpu.py and the error of the float32
restatements against them at n = 1, 3 and B - 1 (printed: the GPU test's bounds rest on these numbers), the oracles following
the dtype of the state they are given, and the trainers' replay / eager / refuse decision as a pure function of shapes."""
import numpy as np
import pytest
import torch

import short_batch_ref as S

CASES = [(name, n) for name in S.MODELS for n in S.sizes(name) if n > 1 or S.SPECS[name].one_ok]


@pytest.mark.parametrize('name,n', CASES)
def test_fp32_reference_stays_inside_a_quarter_of_the_gpu_bound(name, n):
    """The reference alone: float32 against float64 on the first n samples.  Each error is at most a quarter of the bound the
    GPU test uses for that (model, n), and where the model's own bound at batch B already covers 4 x the error that bound
    stands unchanged (`widened` counts the parameters for which it does not)."""
    eloss, egrad = S.fp32_error(name, n)
    bloss, bgrad = S.bounds(name, n)
    assert set(egrad) == set(bgrad) and len(bgrad) > 0
    worst = max(egrad, key=lambda k: egrad[k] / bgrad[k])
    spec = S.SPECS[name]
    widened = [k for k in bgrad if bgrad[k] == 4 * egrad[k] and egrad[k] > 0]
    print(f'{name:10s} n={n:2d}  loss fp32-fp64 {eloss:.2e} (bound {bloss:.1e})  worst gradient {egrad[worst]:.2e} = '
          f'{egrad[worst] / bgrad[worst]:.3f} of its bound ({worst})  widened {len(widened)}/{len(bgrad)}')
    assert eloss <= bloss / 4, (eloss, bloss)
    for k in bgrad:
        assert egrad[k] <= bgrad[k] / 4, (k, egrad[k], bgrad[k])
    assert bloss >= spec.loss_abs + spec.loss_rel * abs(S.reference(name, n).loss)      # never below the model's own bound


@pytest.mark.parametrize('name', [m for m in S.MODELS if m not in ('vqvae', 'cglow')])
def test_restatements_follow_the_dtype_of_their_state(name):
    """float64 state and inputs give a float64 loss and float64 gradients; float32 gives float32 (the one-hot indicator and
    the controller's code follow the state)."""
    for dtype in (torch.float64, torch.float32):
        loss, grads = S.restate(name, 3, dtype)
        assert loss.dtype == dtype and bool(torch.isfinite(loss)), (name, dtype)
        seen = [g for g in grads.values() if g is not None]
        assert len(seen) > 10 and all(g.dtype == dtype for g in seen), (name, dtype)
    assert abs(S.reference(name, 3).loss - S.reference(name, 3, torch.float32).loss) < 1e-5


def test_stored_short_batches_are_consistent():
    """vqvae_train_short.npz / cglow_short.npz: n = 3 whole, the other sizes digests of the same parameters; the float32 and
    float64 runs of the reference picked the same codes (checked when generated) with a decisive arg-min margin."""
    import golden_util as gu
    for name, file in (('vqvae', 'vqvae_train_short.npz'), ('cglow', 'cglow_short.npz')):
        d = gu.load_npz(file)
        whole = S.reference(name, 3)
        assert whole.grads is not None and all(g.dtype == torch.float64 for g in whole.grads.values())
        for n in S.sizes(name):
            r = S.reference(name, n)
            assert sorted(r.grads if r.grads is not None else r.digest) == sorted(whole.grads), (name, n)
            assert np.isfinite(r.loss) and d[f'n{n}/loss'].dtype == np.float64 and d[f'n{n}/loss_fp32'].dtype == np.float32
        if name == 'vqvae':
            assert all(float(d[f'n{n}/dist_margin'].min()) > 1e-4 for n in (1, 3, 7))
            assert d['n3/code'].shape == (3, 8, 8)


def test_a_batch_of_copies_has_the_loss_of_one_sample():
    """Why the broadcast of a one-sample batch into the captured statics was silent: B copies of a sample have the statistics
    of that sample (mean and biased variance over N x H x W), and the losses are batch means -- so loss and gradients equal
    the one-sample step's.  What tells the two apart is the state: the running variance (unbiased, m / (m - 1)) and the
    counts the step accumulates.  test_short_batch_gpu.py therefore pins the statics and the state, not the loss."""
    from oracle import mcpixelcnn_oracle as O
    b = S.batch('mcpixelcnn', 1)
    sd1, sd6 = S._params(S.state('mcpixelcnn'), torch.float64), S._params(S.state('mcpixelcnn'), torch.float64)
    one = O.forward(sd1, b['img'], b['label'], 10, train=True)['loss']
    six = O.forward(sd6, b['img'].expand(6, -1, -1).contiguous(), b['label'].expand(6).contiguous(), 10, train=True)['loss']
    assert abs(float(one.detach()) - float(six.detach())) < 1e-12
    k = 'layers.0.gate_v.bn.running_var'
    assert float((sd1[k] - sd6[k]).abs().max()) > 1e-6


def test_batch_route_is_a_pure_function_of_shapes():
    from mcgen_amd.trainer import batch_route
    statics = [(128, 3, 32, 32), (128,), (128, 3, 32, 32)]
    assert batch_route(statics, statics) == 'replay'
    assert batch_route(statics[:2], [(128, 3, 32, 32), (128,)]) == 'replay'              # (no random input injected)
    assert batch_route([torch.Size(s) for s in statics], [list(s) for s in statics]) == 'replay'
    for n in (1, 3, 80, 127, 129):
        assert batch_route(statics, [(n, 3, 32, 32), (n,), (n, 3, 32, 32)]) == 'eager', n
        assert batch_route(statics[:2], [(n, 3, 32, 32), (n,)]) == 'eager', n
    assert batch_route(None, [(5, 3, 32, 32), (5,)]) == 'eager'                          # nothing captured
    bad = [
        (statics, [(128, 3, 16, 16), (128,), (128, 3, 16, 16)]),        # another resolution, the captured N
        (statics, [(80, 3, 16, 16), (80,), (80, 3, 16, 16)]),           # another resolution, a short N
        (statics, [(80, 1, 32, 32), (80,), (80, 1, 32, 32)]),           # another channel count
        (statics, [(80, 3, 32, 32), (128,), (80, 3, 32, 32)]),          # inputs disagree on N
        (statics, [(128, 3, 32, 32), (1,), (128, 3, 32, 32)]),          # a label that copy_ would broadcast
        (statics, [(1, 3, 32, 32), (1,), (128, 3, 32, 32)]),            # noise of the captured size with a short batch
        (statics[:2], [(80, 3, 32, 32), (80, 1)]),                      # another rank
        (statics[:2], [(80, 3, 32, 32)]),                               # an input missing
        (statics[:2], [(0, 3, 32, 32), (0,)]),                          # an empty batch
        (statics[:2], [(80, 3, 32, 32), ()]),                           # a scalar
        (None, [(5, 3, 32, 32), (4,)]),                                 # nothing captured: N must still agree
    ]
    for st, given in bad:
        with pytest.raises(ValueError, match='Not valid batch'):
            batch_route(st, given)


class _Stub:
    """Stands in for a captured _FlatTrainer on a machine without a GPU: records which path `_dispatch` takes."""
    def __init__(self, statics):
        self.statics, self._graphs, self.calls = statics, True, []

    def _check(self, *inputs):
        pass

    def _draw(self, img, label):
        return torch.zeros(img.shape[0], 4)

    def _replay(self, *inputs, rand=None):
        self.calls.append(('replay', [tuple(t.shape) for t in inputs], None if rand is None else tuple(rand.shape)))

    def _eager(self, *inputs):
        self.calls.append(('eager', [tuple(t.shape) for t in inputs]))


def test_dispatch_on_a_cpu_stub():
    """_FlatTrainer._dispatch over the pure decision: matching shapes replay, a short batch runs eager with the random input
    drawn at the batch's own size, anything else raises before either path is entered."""
    from mcgen_amd.trainer import _FlatTrainer
    st = _Stub([torch.zeros(8, 3, 4, 4), torch.zeros(8, dtype=torch.int64), torch.zeros(8, 4)])
    go = lambda *a, **k: _FlatTrainer._dispatch(st, *a, **k)
    go(torch.zeros(8, 3, 4, 4), torch.zeros(8, dtype=torch.int64))
    go(torch.zeros(8, 3, 4, 4), torch.zeros(8, dtype=torch.int64), rand=torch.ones(8, 4))
    go(torch.zeros(3, 3, 4, 4), torch.zeros(3, dtype=torch.int64))
    go(torch.zeros(1, 3, 4, 4), torch.zeros(1, dtype=torch.int64), rand=torch.ones(1, 4))
    assert st.calls == [('replay', [(8, 3, 4, 4), (8,)], None), ('replay', [(8, 3, 4, 4), (8,)], (8, 4)),
                        ('eager', [(3, 3, 4, 4), (3,), (3, 4)]), ('eager', [(1, 3, 4, 4), (1,), (1, 4)])]
    for img, lab, rand in ((torch.zeros(3, 3, 4, 4), torch.zeros(2, dtype=torch.int64), None),
                           (torch.zeros(3, 3, 8, 8), torch.zeros(3, dtype=torch.int64), None),
                           (torch.zeros(1, 3, 4, 4), torch.zeros(1, dtype=torch.int64), torch.ones(8, 4))):
        with pytest.raises(ValueError, match='Not valid batch'):
            go(img, lab, rand=rand)
    assert len(st.calls) == 4
    before = [t.clone() for t in st.statics]
    assert all(torch.equal(a, b) for a, b in zip(before, st.statics))


def test_vae_training_refuses_one_sample_before_any_launch():
    """MCVAE / CVAE in training mode at N = 1 raise ValueError (the reference's BatchNorm1d raises there): the check comes
    before the engine is touched, so it holds on a machine without a GPU; evaluation mode is not refused by it."""
    from mcgen_amd.vae_engine import check_train_batch
    with pytest.raises(ValueError, match='Not valid batch'):
        check_train_batch(1)
    check_train_batch(2)
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    for name in ('mcvae', 'cvae'):
        cfg.update(model_name=name, data_name='CIFAR10', device='cpu', classes_size=10, controller_rate=0.5, data_shape=[3, 32, 32],
                   compute_dtype='float32')
        cfg['vae'] = {'hidden_size': [8, 16, 32], 'latent_size': 16, 'num_res_block': 2, 'embedding_size': 32}
        m = getattr(models, name)()
        m.train(True)
        b = S.batch(name, 1)
        with pytest.raises(ValueError, match='Not valid batch'):
            m({'img': b['img'], 'label': b['label'], 'eps': b['eps']})
        with torch.no_grad(), pytest.raises(ValueError, match='Not valid batch'):
            m({'img': b['img'], 'label': b['label'], 'eps': b['eps']})
        assert all(p.grad is None for p in m.parameters())
