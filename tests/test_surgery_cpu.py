"""create / transit on the label-embedding baselines, on CPU-built module trees, against the tensors the reference leaves
(tests/golden/surgery_<model>.npz, tools/gen_golden.py: fx_surgery_*), and the float64 Davies-Bouldin restatement
(tests/dbi_ref.py) against scikit-learn's values (tests/golden/dbi.npz).

The surgery is host-side tensor arithmetic (a CPU Dirichlet draw from the fixture's seed, one matmul, numpy's mixing), the
same float32 operations as the reference's, so the comparison is torch.equal."""
import numpy as np
import pytest
import torch

import dbi_ref
import golden_util as gu
import surgery_util as su

BASELINES = ['cgan', 'cvae', 'cglow', 'cpixelcnn']


def _build(name, classes=su.MODES):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    su.configure(name, 'cpu', cfg, classes)
    np.random.seed(0)
    m = getattr(models, name)()
    m.load_state_dict(su.base_state(name), strict=True)
    m.train(False)
    return m, models, cfg


def _assert_state(m, want, what):
    got = m.state_dict()
    assert list(got) == list(want), (what, set(got) ^ set(want))
    for k, v in want.items():
        assert got[k].shape == v.shape and got[k].dtype == v.dtype, (what, k, got[k].shape, v.shape)
        assert torch.equal(got[k], v), (what, k, float((got[k] - v).abs().max()))


@pytest.mark.parametrize('name', BASELINES)
def test_create_reproduces_the_reference(name):
    d = su.load(name)
    m, models, cfg = _build(name)
    names_before = [k for k, _ in m.named_parameters()]
    cfg['classes_size'] = su.NEW_MODES
    torch.manual_seed(int(d['create_seed']))
    with torch.no_grad():
        models.utils.create(m)
    _assert_state(m, su.fixture_state(name, d, 'create'), f'{name} create')
    changed = [k[len('create/'):] for k in d if k.startswith('create/')]
    assert changed and all('embedding' in k for k in changed)
    for k in changed:                                        # swapped in as parameters, stored dense for the gather kernels
        p = dict(m.named_parameters())[k]
        assert isinstance(p, torch.nn.Parameter) and p.is_contiguous()
    new = [k for k, _ in m.named_parameters() if k not in names_before]
    assert new == (['discriminator.embedding.weight'] if name == 'cgan' else [])     # beside the spectral norm's weight_orig
    assert not any(k.endswith('embedding.weight_orig') or k.endswith('conv.weight_orig') for k, _ in m.named_buffers())


@pytest.mark.parametrize('name', ['cgan', 'cvae', 'cglow'])
def test_transit_reproduces_the_reference(name):
    d = su.load(name)
    m, models, cfg = _build(name)
    for i, alpha in enumerate(d['alphas'].tolist()):         # successive calls on one model, as transit.py makes them
        with torch.no_grad():
            models.utils.transit(m, int(d['root']), alpha)
        _assert_state(m, su.fixture_state(name, d, f'transit{i}'), f'{name} transit alpha={alpha}')
    base = su.base_state(name)
    buffers = dict(m.named_buffers())
    kept = [k for k in buffers if k.endswith('weight_orig')]
    assert kept and all(torch.equal(buffers[k], base[k[:-len('_orig')]]) for k in kept)      # the original, kept as a buffer
    if name == 'cgan':                                       # the spectral norm's weight_orig is reused, not shadowed
        emb = m.discriminator.embedding
        assert 'weight_orig' in emb._parameters and 'weight_orig' not in emb._buffers
        assert torch.equal(emb.weight_orig, base['discriminator.embedding.weight_orig'])


def test_transit_with_numpy_alphas_keeps_float32_tables():
    """transit.py hands over np.linspace's float64 scalars: the tables stay float32 and equal the Python-float result."""
    d = su.load('cvae')
    m, models, cfg = _build('cvae')
    for i, alpha in enumerate(np.linspace(0, 1, 3)):
        with torch.no_grad():
            models.utils.transit(m, int(d['root']), alpha)
        _assert_state(m, su.fixture_state('cvae', d, f'transit{i}'), f'cvae transit alpha={alpha!r}')


def test_transit_leaves_cpixelcnn_tables():
    m, models, cfg = _build('cpixelcnn')
    before = {k: v.clone() for k, v in m.state_dict().items()}
    models.utils.transit(m, su.ROOT, 0.5)
    _assert_state(m, before, 'cpixelcnn transit')


def test_counts_follow_the_live_tables():
    """The host-side label bounds after create (10 -> 14 and 10 -> 6) come from the tables' shapes; a training-mode call and
    CGAN's discriminator are refused with a ValueError that names the mismatch.  Nothing here launches a kernel."""
    from mcgen_amd import pixelcnn_sampler
    from mcgen_amd.models.cpixelcnn import table_modes
    for new in (14, 6):
        for name in BASELINES:
            m, models, cfg = _build(name)
            cfg['classes_size'] = new
            models.utils.create(m)
            ok, bad = torch.tensor([0, new - 1]), [torch.tensor([new]), torch.tensor([new + 3]), torch.tensor([-1])]
            if name == 'cgan':
                assert m.generator.table_modes(False) == new
                check = lambda lab: m._labels(lab, m.generator)                     # noqa: E731
                with pytest.raises(ValueError, match='weight_orig'):
                    m.discriminate(torch.zeros(2, 3, 32, 32), ok)
            elif name == 'cpixelcnn':
                assert table_modes(m) == new and pixelcnn_sampler.num_modes(m) == new
                check = lambda lab: pixelcnn_sampler.validate(m, lab)               # noqa: E731
            else:
                check = m._label
            check(ok)
            for lab in bad:
                with pytest.raises(ValueError):
                    check(lab)
            m.train(True)
            with pytest.raises(ValueError, match=f'{new} modes'):
                if name == 'cgan':
                    m.generate(ok, torch.zeros(2, 128))
                elif name == 'cpixelcnn':
                    m({'img': torch.zeros(2, 8, 8, dtype=torch.long), 'label': ok})
                else:
                    m({'img': torch.zeros(2, 3, 32, 32), 'label': ok})


def test_tables_that_disagree_are_refused():
    m, models, cfg = _build('cpixelcnn')
    m.layers[2].class_cond_embedding.weight = torch.nn.Parameter(torch.zeros(6, 32))
    from mcgen_amd import pixelcnn_sampler
    with pytest.raises(ValueError, match='disagree'):
        pixelcnn_sampler.validate(m, torch.tensor([0]))
    v, models, cfg = _build('cvae')
    v.encoder.embedding.weight = torch.nn.Parameter(torch.zeros(32, 6))
    v._label(torch.tensor([9]), encoder=False)               # generate gathers from the decoder's table alone
    with pytest.raises(ValueError, match='disagree'):
        v._label(torch.tensor([0]))


@pytest.mark.parametrize('name', ['mcgan', 'mcvae', 'mcglow', 'mcpixelcnn'])
def test_mc_models_are_handled_as_before(name):
    """The MultimodalController branches: a fresh codebook of cfg['classes_size'] rows from create, codebook_orig and a spliced
    codebook from transit; no embedding appears."""
    from mcgen_amd import models
    from mcgen_amd.config import cfg, process_control
    cfg.update(model_name=name, data_name='CIFAR10', device='cpu', control={'controller_rate': '0.5'})
    cfg.pop('classes_size', None)
    process_control()
    if 'gan' in name:
        cfg['gan']['generator_hidden_size'], cfg['gan']['discriminator_hidden_size'] = [32] * 4, [16] * 4
    elif 'vae' in name:
        cfg['vae'].update(hidden_size=[8, 16, 32], latent_size=16)
    elif 'glow' in name:
        cfg['glow'].update(hidden_size=32, K=2, L=3)
    else:
        cfg['pixelcnn'].update(num_layer=4, hidden_size=16, num_embedding=32)
    np.random.seed(0)
    torch.manual_seed(0)
    m = getattr(models, name)()
    mcs = [mod for mod in m.modules() if mod.__class__.__name__ == 'MultimodalController']
    assert mcs
    widths = [mc.codebook.shape[1] for mc in mcs]
    keys = list(m.state_dict())
    models.utils.transit(m, 2, 0.5)
    for mc, w in zip(mcs, widths):
        cross = int(round(0.5 * w))
        assert tuple(mc.codebook.shape) == (10, w) and torch.equal(mc.codebook[2], mc.codebook_orig[2])
        assert all(torch.equal(mc.codebook[i, :cross], mc.codebook_orig[2, :cross]) for i in range(10))
        assert torch.equal(mc.codebook[:, cross:], mc.codebook_orig[:, cross:])
    assert [k for k in m.state_dict() if k not in keys] == [k for k in m.state_dict() if k.endswith('codebook_orig')]
    cfg['classes_size'] = 14
    models.utils.create(m)
    assert all(tuple(mc.codebook.shape) == (14, w) for mc, w in zip(mcs, widths))
    assert not any('embedding' in k and 'weight_orig' in k for k in m.state_dict())
    cfg['classes_size'] = 10


# ---- Davies-Bouldin restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(dbi_ref.CASES))
def test_dbi_ref_matches_scikit_learn(case):
    """float64 sums of at most 3072 * N terms in another order than scikit-learn's: forward error below n * 2^-53 ~ 1e-12."""
    d = gu.load_npz('dbi.npz')
    x, label = dbi_ref.make_case(case)
    assert list(d[case + '/shape_seed']) == list(dbi_ref.CASES[case])
    assert [float(x.astype(np.float64).sum()), float(label.sum())] == d[case + '/checksum'].tolist()     # the fixture's inputs
    got, want = dbi_ref.reference(case), float(d[case + '/sklearn_f64'])
    print(case, got, want, float(d[case + '/sklearn_f32']))
    assert abs(got - want) <= 1e-12 * want
    assert abs(float(d[case + '/sklearn_f32']) - want) <= 1e-6 * want


def test_dbi_ref_degenerate_and_errors():
    x, label = dbi_ref.make_case('uneven')
    assert dbi_ref.davies_bouldin(np.ones_like(x), label) == 0.0                     # every spread and distance zero
    same_centre = np.concatenate([x[:10], x[:10]])                                   # two clusters, one centroid
    assert dbi_ref.davies_bouldin(same_centre, np.repeat([0, 1], 10)) == 0.0
    with pytest.raises(ValueError):
        dbi_ref.davies_bouldin(x, np.zeros_like(label))                              # one cluster
    with pytest.raises(ValueError):
        dbi_ref.davies_bouldin(x, np.arange(len(x)))                                 # as many clusters as samples
    # an absent label id is no cluster: relabelling with gaps changes nothing
    assert dbi_ref.davies_bouldin(x, label * 5 + 2) == dbi_ref.davies_bouldin(x, label)
