"""The three forms a captured MCGAN step takes -- (a) the whole loop body as one graph, (b) per-bucket graphs around a
grouped 5 N generator pass (what a multi-rank run replays; on one rank only with `_ONE_GRAPH` off), (c) per-bucket graphs
with one generator pass per discriminator update -- each against the eager trainer under the same flags.

Reduced width, 10 modes, fp32, N = 128: the smallest batch at which `fake_groups` is 5.  The bound is the one
test_mcgan_gpu.py::test_graphed_trainer_matches_eager holds the replayed state to: 1e-6 + 1e-5 max|v|.
"""
import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu

N, MODES, G_HIDDEN, D_HIDDEN = 128, 10, [32] * 4, [16] * 4


@pytest.fixture(scope='module')
def inputs():
    sd = gu.procedural_state(gu.mcgan_shapes(G_HIDDEN, D_HIDDEN, MODES), seed=31, num_mode=MODES)
    img, lab = gu.synthetic_batch(N, MODES, seed=5)
    zs = [z.cuda() for z in gu.latent_batches(12, N, 128, seed=6)]
    return sd, img.cuda(), lab.cuda(), zs


def _build(sd):
    from mcgen_amd import models
    from mcgen_amd.config import cfg, process_control
    cfg['data_name'], cfg['model_name'], cfg['device'] = 'CIFAR10', 'mcgan', 'cuda'
    cfg.pop('classes_size', None)
    process_control()
    cfg['classes_size'] = MODES
    cfg['gan']['generator_hidden_size'], cfg['gan']['discriminator_hidden_size'] = list(G_HIDDEN), list(D_HIDDEN)
    m = models.mcgan()
    m.load_state_dict(sd)
    return m.cuda().set_compute_dtype(torch.float32)


def _is_one_graph(tr):
    assert tr.g_all is not None and tr._fg == 5


def _is_bucketed_grouped(tr):
    assert tr.g_all is None and tr._fg == 5
    assert len(tr.g_dc) == 5 and len(tr.g_da) == 5              # a set of D graphs per batch of the grouped pass


def _is_bucketed(tr):
    assert tr.g_all is None and tr._fg == 5


def _is_bucketed_per_update(tr):
    assert tr.g_all is None and tr._fg == 1


# (the last two: the same forms with the engine-to-engine images going through NCHW fp32, `_NHWC_PAIR` off)
@pytest.mark.parametrize('flags,is_form', [((), _is_one_graph), (('_ONE_GRAPH',), _is_bucketed_grouped),
                                           (('_GROUP_G',), _is_bucketed_per_update), (('_NHWC_PAIR',), _is_one_graph),
                                           (('_NHWC_PAIR', '_ONE_GRAPH'), _is_bucketed)],
                         ids=['one_graph', 'bucketed', 'per_update', 'one_graph_nchw', 'bucketed_nchw'])
def test_replay_form_matches_eager(inputs, flags, is_form):
    from mcgen_amd import trainer as T
    sd, img, lab, zs = inputs
    old = {f: getattr(T, f) for f in flags}
    for f in flags:
        setattr(T, f, False)
    try:
        m = _build(sd)
        tr = T.GraphedGANTrainer(m, MODES)
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        tr.capture(img, lab)
        torch.cuda.synchronize()
        assert tr._graphs is not None
        is_form(tr)
        # capture leaves the model, the moments and the counters exactly as they were
        for k, v in m.state_dict().items():
            assert torch.equal(v, before[k]), k
        for opt in (tr.opt_d, tr.opt_g):
            assert int(opt.step_count) == 0
            assert float(opt.m.abs().max()) == 0.0 and float(opt.v.abs().max()) == 0.0
        # memory taken after the capture is not the graphs' to write: a snapshot's copies survive the replays
        _, kept = tr.device_snapshot()
        kept_host = [t.cpu() for t in kept]

        def two_iterations(t):      # (a replay returns the graph's own loss tensors: read them before the next one)
            return [tuple(float(v) for v in t.train_iteration(img, lab, zs[6 * it:6 * it + 6])) for it in range(2)]
        got = two_iterations(tr)
        for i, (t, h) in enumerate(zip(kept, kept_host)):
            assert torch.equal(t.cpu(), h), f'replay wrote into snapshot tensor {i}'
        m2 = _build(sd)
        te = T.GANTrainer(m2, MODES)
        ref = two_iterations(te)
        print(f'{flags}: replayed losses {got}, eager {ref}')
        for a, b in zip(np.ravel(got), np.ravel(ref)):
            assert abs(a - b) <= 1e-6 + 1e-5 * abs(b), (got, ref)
        sd_g, sd_e = m.state_dict(), m2.state_dict()
        for k, v in sd_e.items():
            if v.dtype == torch.int64:
                assert int(sd_g[k]) == int(v), k
            else:
                assert float((sd_g[k] - v).abs().max()) <= 1e-6 + 1e-5 * float(v.abs().max()), k
        for t in (tr, te):
            assert int(t.opt_d.step_count) == 10 and int(t.opt_g.step_count) == 2
        for name in ('opt_d', 'opt_g'):
            for slot in ('m', 'v'):
                a, b = getattr(getattr(tr, name), slot), getattr(getattr(te, name), slot)
                assert float((a - b).abs().max()) <= 1e-6 + 1e-5 * float(b.abs().max()), (name, slot)
        dl, gl = tr.train_iteration(img, lab)                      # no `zs`: the replay draws its own latents
        assert np.isfinite(float(dl)) and np.isfinite(float(gl))
    finally:
        for f, v in old.items():
            setattr(T, f, v)
