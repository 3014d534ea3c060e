"""create / transit on the HIP path: eval-mode generate / sample of the four label-embedding baselines on the tensors the
reference's surgery leaves (tests/golden/surgery_<model>.npz) against the reference's outputs, the transit endpoints for the
baselines and the MultimodalController models, and the host-side label bounds after a create that changes the mode count.
Tolerances are those of each model's existing eval-generate test (test_cgan_gpu 2e-4, test_cvae_gpu / test_mcvae_gpu 5e-4,
test_cglow_gpu / test_mcglow_gpu 1e-3, test_mcgan_gpu 2e-4, test_cpixelcnn_gpu 5e-4 on logits and equal greedy decodes)."""
import numpy as np
import pytest
import torch

import golden_util as gu
import surgery_util as su

pytestmark = pytest.mark.gpu

BASELINES = ['cgan', 'cvae', 'cglow', 'cpixelcnn']
TOL = {'cgan': 2e-4, 'cvae': 5e-4, 'cglow': 1e-3, 'cpixelcnn': 5e-4, 'mcgan': 2e-4, 'mcvae': 5e-4, 'mcglow': 1e-3}


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b)).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _baseline(name):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    su.configure(name, 'cuda', cfg)
    np.random.seed(0)
    m = getattr(models, name)()
    m.load_state_dict(su.base_state(name), strict=True)
    m = m.cuda()
    m.train(False)
    return m


def _mc_model(name):
    """(model in eval mode on the reference's trained state of its *_small fixture, modes, latent shapes)."""
    from mcgen_amd import models
    from mcgen_amd.config import cfg, process_control
    d = gu.load_npz(f'{name}_small.npz')
    if name == 'mcgan':
        cfg.update(data_name='CIFAR10', model_name='mcgan', device='cuda')
        cfg.pop('classes_size', None)
        process_control()
        cfg['gan']['generator_hidden_size'], cfg['gan']['discriminator_hidden_size'] = [32] * 4, [16] * 4
        modes, shapes = 10, (128,)
    elif name == 'mcvae':
        cfg.update(model_name='mcvae', data_name='CIFAR10', device='cuda', classes_size=10, controller_rate=0.5,
                   data_shape=[3, 32, 32], compute_dtype='float32')
        cfg['vae'] = {'hidden_size': [8, 16, 32], 'latent_size': 16, 'num_res_block': 2, 'embedding_size': 32}
        modes, shapes = 10, (16,)
    else:
        cfg.update(model_name='mcglow', device='cuda', classes_size=12, controller_rate=0.5, data_shape=[1, 32, 32],
                   compute_dtype='float32')
        cfg['glow'] = {'hidden_size': 32, 'K': 2, 'L': 3, 'affine': True, 'conv_lu': True}
        modes, shapes = 12, [(2, 16, 16), (4, 8, 8), (16, 4, 4)]
    np.random.seed(0)
    m = getattr(models, name)()
    m.load_state_dict(gu.state_from_npz(d, 'sd_final/'))
    m = m.cuda()
    m.train(False)
    return m, modes, shapes


def _install(m, state):
    """Put the fixture's tensors into the module tree the way the surgery does: a replaced `weight` as a new nn.Parameter, a
    kept original as the `weight_orig` buffer."""
    have = m.state_dict()
    for k, v in state.items():
        if k in have and have[k].shape == v.shape and torch.equal(have[k].cpu(), v):
            continue
        path, leaf = k.rsplit('.', 1)
        mod = m.get_submodule(path)
        if leaf == 'weight':
            mod.weight = torch.nn.Parameter(v.cuda())
        else:
            assert leaf == 'weight_orig' and leaf not in mod._parameters, k
            mod.register_buffer(leaf, v.cuda())
    assert list(m.state_dict()) == list(state)


def _to(x):
    return [t.cuda() for t in x] if isinstance(x, list) else x.cuda()


# ---- parity with the reference on the fixture's states ----------------------------------------------------------------------
@pytest.mark.parametrize('name', BASELINES)
def test_generate_on_the_reference_states(name):
    d = su.load(name)
    tags = ['create'] + ([] if name == 'cpixelcnn' else ['transit0', 'transit1', 'transit2'])
    for tag in tags:
        m = _baseline(name)
        _install(m, su.fixture_state(name, d, tag))
        label, x = su.inputs(name, su.NEW_MODES if tag == 'create' else su.MODES)
        with torch.no_grad():
            if name == 'cpixelcnn':
                greedy = torch.from_numpy(d[f'{tag}_out/greedy'])
                got, logits = m.sample(label.cuda(), greedy=True, return_logits=True)
                err = _rel(logits, d[f'{tag}_out/logits'])
                print(name, tag, 'logits', err)
                assert torch.equal(got.cpu(), greedy)
                assert err < TOL[name]
                assert torch.equal(m.generate(label.cuda(), sampler=lambda p: p.argmax(-1)).cpu(), greedy)
            else:
                gen = m.generate(label.cuda(), _to(x))
                err = _rel(gen, d[f'{tag}_out/gen'])
                print(name, tag, err)
                assert gen.shape == d[f'{tag}_out/gen'].shape and err < TOL[name]


# ---- transit endpoints ----------------------------------------------------------------------------------------------------------
def _same_rows(shapes, n, seed=5):
    g = torch.Generator().manual_seed(seed)
    if isinstance(shapes, list):
        return [torch.randn(1, *s, generator=g).mul(0.7).expand(n, *s).contiguous().cuda() for s in shapes]
    return torch.randn(1, *shapes, generator=g).expand(n, *shapes).contiguous().cuda()


@pytest.mark.parametrize('name', ['cgan', 'cvae', 'cglow', 'mcgan', 'mcvae', 'mcglow'])
def test_transit_endpoints(name):
    """On one latent for every mode: alpha = 0 makes every mode the root, alpha = 1 is the untouched model bit for bit."""
    from mcgen_amd.models import utils as mu
    if name.startswith('mc'):
        m, modes, shapes = _mc_model(name)
    else:
        m, modes = _baseline(name), su.MODES
        shapes = {'cgan': (128,), 'cvae': (16,), 'cglow': [(6, 16, 16), (12, 8, 8), (48, 4, 4)]}[name]
    C, x = torch.arange(modes).cuda(), _same_rows(shapes, modes)
    with torch.no_grad():
        base = m.generate(C, x).clone()
        mu.transit(m, su.ROOT, 0.0)
        at0 = m.generate(C, x).clone()
        mu.transit(m, su.ROOT, 1.0)
        at1 = m.generate(C, x).clone()
    assert float((base - base[su.ROOT:su.ROOT + 1]).abs().max()) > 1e-3            # the modes differ to begin with
    err = _rel(at0, at0[su.ROOT:su.ROOT + 1].expand_as(at0))
    print(name, 'alpha 0', err, 'root', _rel(at0[su.ROOT], base[su.ROOT]))
    assert err < TOL[name] and _rel(at0[su.ROOT], base[su.ROOT]) < TOL[name]
    assert torch.equal(at1, base)


# ---- a create that changes the number of modes -----------------------------------------------------------------------------
@pytest.mark.parametrize('new', [6, 14])
@pytest.mark.parametrize('name', BASELINES)
def test_fewer_and_more_modes(name, new):
    """Labels up to the new maximum run; the first label past the table, and one three past it, are refused on the host (these
    calls never reach a launch); training mode and CGAN's discriminator are refused too."""
    from mcgen_amd.config import cfg
    from mcgen_amd.models import utils as mu
    m = _baseline(name)
    cfg['classes_size'] = new
    torch.manual_seed(1)
    mu.create(m)
    cfg['classes_size'] = su.MODES
    C = torch.arange(new).cuda()
    _, x = su.inputs(name, new)
    run = (lambda lab: m.sample(lab, greedy=True, return_logits=True)[1]) if name == 'cpixelcnn' else \
        (lambda lab: m.generate(lab, _to([t[:1].expand(lab.numel(), *t.shape[1:]).contiguous() for t in x] if isinstance(x, list)
                                         else x[:1].expand(lab.numel(), -1).contiguous())))
    with torch.no_grad():
        out = run(C)
    assert out.shape[0] == new and bool(torch.isfinite(out.float()).all())
    assert len({out[i].cpu().numpy().tobytes() for i in range(new)}) == new       # every label reaches its own table entry
    for bad in (new, new + 3):
        with pytest.raises(ValueError):
            run(torch.tensor([0, bad]).cuda())
    if name == 'cgan':
        with pytest.raises(ValueError, match='weight_orig'):
            m.discriminate(torch.zeros(new, 3, 32, 32).cuda(), C)
    m.train(True)
    with pytest.raises(ValueError):
        if name == 'cgan':
            m.generate(C, torch.zeros(new, 128).cuda())
        elif name == 'cpixelcnn':
            m({'img': torch.zeros(new, 8, 8, dtype=torch.long).cuda(), 'label': C})
        else:
            m({'img': torch.zeros(new, 3, 32, 32).cuda(), 'label': C})


def test_cgan_generator_rebinds_to_the_replaced_parameter():
    from mcgen_amd.config import cfg
    from mcgen_amd.models import utils as mu
    m = _baseline('cgan')
    label, x = su.inputs('cgan', su.MODES)
    with torch.no_grad():
        before = m.generate(label.cuda(), x.cuda()).clone()                          # builds the engine on the old parameter set
        eng = m.generator._engine()
        cfg['classes_size'] = 14
        mu.create(m)
        cfg['classes_size'] = su.MODES
        m.generate(torch.tensor([13]).cuda(), x[:1].cuda())
        assert any(p is m.generator.embedding.weight for p in eng.flat_p.tensors)
        assert [tuple(p.shape) for p in eng.flat_p.tensors] == [tuple(p.shape) for p in m.generator.parameters()]
        mu.transit(m, su.ROOT, 1.0)                                                  # 14 modes still; alpha 1 changes nothing
        again = m.generate(torch.tensor([13]).cuda(), x[:1].cuda())
        assert any(p is m.generator.embedding.weight for p in eng.flat_p.tensors) and bool(torch.isfinite(again).all())
    assert bool(torch.isfinite(before).all())


def test_sampler_after_create_follows_the_new_tables():
    """The counterpart of test_pixelcnn_sample_gpu's MultimodalController test: 4 new modes, the incremental sampler's logits
    equal one eval-mode forward of the drawn map on the new tables, and the old labels are refused."""
    from mcgen_amd.config import cfg
    from mcgen_amd.models import utils as mu
    m = _baseline('cpixelcnn')
    cfg['classes_size'] = 4
    torch.manual_seed(0)
    mu.create(m)
    cfg['classes_size'] = su.MODES
    assert all(L.class_cond_embedding.weight.shape == (4, 32) for L in m.layers)
    lab = (torch.arange(20) % 4).cuda()
    x, lg = m.sample(lab, return_logits=True)
    with torch.no_grad():
        ref = m({'img': x, 'label': lab})['logits']
    assert _rel(lg, ref.float()) < 2e-5
    with pytest.raises(ValueError, match='Not valid'):
        m.sample(torch.full((3,), 5, dtype=torch.long, device='cuda'))
