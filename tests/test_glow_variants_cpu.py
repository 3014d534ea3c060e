"""MCGlow with additive coupling and / or the plain InvConv2d (cfg glow.affine / glow.conv_lu = False): module surface and
reference checkpoints, the library surface, the drivers' --glow_affine / --glow_conv_lu flags, and the float64 restatement
(tests/glow_variants_ref.py) against the reference-generated fixtures.  CPU only."""
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import glow_variants_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def glow_cfg():
    from mcgen_amd.config import cfg
    saved = {k: v for k, v in cfg.items()}

    def set_(name, classes, channels, affine, conv_lu):
        cfg.update(model_name=name, device='cpu', classes_size=classes, data_shape=[channels, 32, 32], controller_rate=0.5)
        cfg['glow'] = R.glow_cfg(affine, conv_lu)
        return cfg
    yield set_
    cfg.clear()
    cfg.update(saved)


@pytest.mark.parametrize('fixture,classes,channels,affine,conv_lu', R.FIXTURES)
def test_state_dict_layout_and_strict_load(glow_cfg, fixture, classes, channels, affine, conv_lu):
    """The reference's constructor arguments construct, and its state_dict (keys, order, shapes, dtypes) loads strictly."""
    from mcgen_amd import models
    d = R.load(fixture)
    shapes = R.layout(d)
    glow_cfg('mcglow', classes, channels, affine, conv_lu)
    np.random.seed(0); torch.manual_seed(0)
    m = models.mcglow()
    own = m.state_dict()
    assert list(own) == list(shapes)
    assert {k: tuple(v.shape) for k, v in own.items()} == shapes
    sd0, init, final = R.states(d)
    for k, v in sd0.items():
        assert own[k].dtype == v.dtype, k
    c = 4 * channels
    for b in range(R.L):
        for f in range(R.K):
            pre = f'blocks.{b}.flows.{f}.'
            if conv_lu:
                assert shapes[pre + 'invconv.w_s'] == (c,) and pre + 'invconv.weight' not in shapes
            else:                                            # one parameter, no buffers (mcglow.py:58-64)
                assert [k for k in shapes if k.startswith(pre + 'invconv.')] == [pre + 'invconv.weight']
                assert shapes[pre + 'invconv.weight'] == (c, c, 1, 1)
            assert shapes[pre + 'coupling.net.8.module.conv.weight'] == (c if affine else c // 2, R.HIDDEN, 3, 3)
            assert shapes[pre + 'coupling.net.8.module.scale'] == (1, c if affine else c // 2, 1, 1)
        c *= 2
    for sd in (sd0, init, final):
        m.load_state_dict(sd, strict=True)
    if not conv_lu:                                          # a fresh InvConv2d starts orthogonal (the Q of a random matrix)
        w = models.mcglow().blocks[1].flows[0].invconv.weight.detach()[:, :, 0, 0].double()
        assert float((w @ w.T - torch.eye(w.shape[0], dtype=torch.float64)).abs().max()) < 1e-5
    assert [tuple(s) for s in m.make_z_shapes()] == [(2 * channels, 16, 16), (4 * channels, 8, 8), (16 * channels, 4, 4)]
    names = {k for k, _ in m.named_parameters()}             # the trainer's flat buffers run over parameters(): the weight is one
    assert ('blocks.0.flows.0.invconv.weight' in names) == (not conv_lu)


def test_variants_do_not_load_into_each_other(glow_cfg):
    """model_tag stays the reference's: a checkpoint of another variant fails the strict load."""
    from mcgen_amd import models
    glow_cfg('mcglow', 12, 1, True, True)
    np.random.seed(0)
    m = models.mcglow()
    for fixture, *_ in R.FIXTURES[:2]:
        with pytest.raises(RuntimeError):
            m.load_state_dict(R.states(R.load(fixture))[0], strict=True)


def test_cglow_still_refuses_unbuilt_forms(glow_cfg):
    from mcgen_amd import models
    for key in ('affine', 'conv_lu'):
        glow_cfg('cglow', 12, 1, key != 'affine', key != 'conv_lu')
        with pytest.raises(ValueError):
            models.cglow()


def test_fixtures_exercise_the_variants():
    """No NaN (loss_fn zeroes NaN samples: one would hide errors), a repeated label and the last mode, non-zero ZeroConv2d
    tensors, and a log-determinant term W^-T that is not negligible against the bare dW in the plain weight's gradient."""
    for fixture, classes, _, affine, conv_lu in R.FIXTURES:
        d = R.load(fixture)
        for k, v in d.items():
            assert v.dtype.kind != 'f' or np.isfinite(v).all(), k
        lab = d['label']
        assert len(set(lab.tolist())) < len(lab) and classes - 1 in lab
        assert float(np.abs(d['sd/blocks.0.flows.0.coupling.net.8.module.conv.weight']).max()) > 0
        assert float(np.abs(d['grad0/blocks.1.flows.1.coupling.net.0.module.weight']).max()) > 0
        if not conv_lu:
            n, npix = len(lab), float(d['img'][0].size)
            for b, hw in enumerate((256, 64, 16)):
                k = f'blocks.{b}.flows.1.invconv.weight'
                w = torch.from_numpy(d['sd/' + k])[:, :, 0, 0].double()
                term = -hw / (np.log(2.) * npix) * torch.linalg.inv(w).T          # d loss / d W through H W log|det W|
                g = torch.from_numpy(d['grad0/' + k])[:, :, 0, 0].double()
                assert float(term.abs().max()) > 0.1 * float(g.abs().max()), k
                assert float((w @ w.T - torch.eye(w.shape[0], dtype=torch.float64)).abs().max()) > 0.1     # not orthogonal


@pytest.mark.parametrize('fixture,classes,channels,affine,conv_lu', R.FIXTURES)
def test_float64_restatement_reproduces_the_fixture(fixture, classes, channels, affine, conv_lu):
    """Guards the helper the GPU tests lean on: the float64 likelihood written from the formulas gives the reference's first
    logged loss and its first-step gradients of the 1x1 convolution's parameters (invconv.weight; the LU fixture: w_s,
    w_l, w_u) within the bounds the GPU tests put on the kernels (loss 1e-4, gradients 2e-4 max|g| + 1e-6): the
    reference ran in fp32, the restatement in float64."""
    d = R.load(fixture)
    _, init, _ = R.states(d)
    leaves = ('w_s', 'w_l', 'w_u') if conv_lu else ('weight',)
    wanted = [f'blocks.{b}.flows.{f}.invconv.{leaf}' for b in range(R.L) for f in range(R.K) for leaf in leaves]
    wanted.append('blocks.0.flows.0.coupling.net.8.module.scale')
    loss, grads = R.loss_and_grads(init, torch.from_numpy(d['img']), torch.from_numpy(d['label']),
                                   torch.from_numpy(d['noise/0/0']), wanted)
    print('loss', loss, float(d['losses'][0]))
    assert abs(loss - float(d['losses'][0])) < 1e-4
    for k in wanted:
        ref = torch.from_numpy(d['grad0/' + k]).double()
        g = grads[k]
        if k.endswith('w_l'):                                # the reference masks the factors: no gradient off the triangle
            g = g * torch.tril(torch.ones_like(g), -1)
        if k.endswith('w_u'):
            g = g * torch.triu(torch.ones_like(g), 1)
        err, tol = float((g - ref).abs().max()), 2e-4 * float(ref.abs().max()) + 1e-6
        assert err < tol, (k, err, tol)


# ---- library surface -------------------------------------------------------------------------------------------------------------
def test_library_exports_variant_kernels():
    from mcgen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = ('mcgen_invconv_plain', 'mcgen_invconv_plain_batch', 'mcgen_invconv_plain_bwd', 'mcgen_invconv_plain_bwd_batch',
             'mcgen_glow_coupling_add')
    for name in names:
        assert hasattr(raw, name) and name in _lib.SYMBOLS and name in _lib.HEADER.functions, name
    assert 'glow_variants' in open(os.path.join(ROOT, 'multimodal-controller-for-generative-models_amd', 'csrc', 'build.sh')).read()
    assert ctypes.sizeof(_lib.Icp) == 32 and ctypes.sizeof(_lib.Icpb) == 40
    # host-side argument checks, before any launch
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for c in (0, -1, 65):
        assert lib.mcgen_invconv_plain(p, c, p, p, None) != 0
        assert b'invconv_plain' in lib.mcgen_last_error()
        assert lib.mcgen_invconv_plain_bwd(p, c, 72, p, 1.0, p, 0, None) != 0
    assert lib.mcgen_invconv_plain(None, 4, p, p, None) != 0
    assert lib.mcgen_invconv_plain_bwd(p, 8, 7, p, 1.0, p, 0, None) != 0                   # row pitch below C
    job = (_lib.Icp * 2)()
    for j in job:
        j.weight, j.logabsdet, j.weight_inv, j.C = p, p, p, 4
    job[1].C = 65
    assert lib.mcgen_invconv_plain_batch(job, 2, None) != 0 and b'job 1' in lib.mcgen_last_error()
    assert lib.mcgen_invconv_plain_batch(job, 0, None) != 0
    add = lib.mcgen_glow_coupling_add
    assert add(p, p, p, 0, 4, 5, 8, 8, 1, None) != 0                                       # odd C
    assert add(p, p, p, 0, 4, 12, 8, 8, 1, None) != 0                                      # Cp below C
    assert add(p, p, p, 0, 4, 12, 12, 8, 1, None) != 0                                     # Cp no multiple of 8
    assert add(p, p, p, 0, 4, 12, 16, 4, 1, None) != 0                                     # h narrower than C / 2
    assert add(p, p, p, 0, 4, 12, 16, 8, 0, None) != 0                                     # sign is +1 or -1
    assert add(p, p, p, 7, 4, 12, 16, 8, 1, None) != 0                                     # no such dtype
    assert b'coupling_add' in lib.mcgen_last_error() or b'dtype' in lib.mcgen_last_error()


def test_wrappers_have_no_cpu_path():
    from mcgen_amd import _lib, ops
    w = torch.eye(4)
    with pytest.raises(_lib.McgenError):
        ops.invconv_plain(w)
    with pytest.raises(_lib.McgenError):
        ops.glow_coupling_add(torch.zeros(1, 2, 2, 8), torch.zeros(1, 2, 2, 8), 4)


# ---- the drivers' flags ----------------------------------------------------------------------------------------------------------
def _flags():
    spec = importlib.util.spec_from_file_location('_mcgen_compat_flags', os.path.join(ROOT, 'compat', '_flags.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_glow_flags_parse_and_apply():
    fl = _flags()
    table = {'hidden_size': 512, 'K': 16, 'L': 3, 'affine': True, 'conv_lu': True}
    argv = ['x.py', '--glow_affine', 'False', '--data_name', 'CIFAR10', '--glow_conv_lu=False']
    flags = fl.pop_glow_flags(argv)
    assert flags == {'affine': False, 'conv_lu': False} and argv == ['x.py', '--data_name', 'CIFAR10']
    cfg = {'model_name': 'mcglow', 'glow': dict(table)}
    fl.apply_glow_flags(cfg, flags)
    assert cfg['glow'] == dict(table, affine=False, conv_lu=False)
    # the default leaves the table untouched (the same object: nothing was applied)
    argv = ['x.py', '--data_name', 'CIFAR10']
    cfg = {'model_name': 'mcglow', 'glow': table}
    fl.apply_glow_flags(cfg, fl.pop_glow_flags(argv))
    assert cfg['glow'] is table and argv == ['x.py', '--data_name', 'CIFAR10']
    # one flag alone, and an explicit True
    cfg = {'model_name': 'mcglow', 'glow': dict(table)}
    fl.apply_glow_flags(cfg, fl.pop_glow_flags(['x.py', '--glow_conv_lu', 'False', '--glow_affine', 'True']))
    assert cfg['glow'] == dict(table, conv_lu=False)
    # cglow: a False is refused with the constructor's message, a True is the table
    for key, word in (('affine', 'coupling'), ('conv_lu', 'invertible conv')):
        with pytest.raises(ValueError, match='Not valid ' + word):
            fl.apply_glow_flags({'model_name': 'cglow', 'glow': dict(table)}, {key: False})
    cfg = {'model_name': 'cglow', 'glow': dict(table)}
    fl.apply_glow_flags(cfg, {'affine': True})
    assert cfg['glow'] == table
    with pytest.raises(ValueError):
        fl.pop_glow_flags(['x.py', '--glow_affine', 'no'])
    with pytest.raises(ValueError):
        fl.apply_glow_flags({'model_name': 'mcvae'}, {'affine': False})


_PROBE = r'''
import json, sys
sys.path.insert(0, {compat!r})
sys.argv = ['train_glow.py'] + {args!r}
import train_glow as T
import _single
captured = {{}}
def fake_run(self):
    cfg = _single.cfg
    captured.update(tag=cfg['model_tag'], glow=cfg['glow'])
T.GlowDriver.run_experiment = fake_run
try:
    T.main()
except ValueError as e:
    captured['error'] = str(e)
print(json.dumps(captured))
'''


def _probe(args, tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    code = _PROBE.format(compat=os.path.join(ROOT, 'compat'), args=args)
    r = subprocess.run([sys.executable, '-c', code], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_train_glow_driver_applies_the_flags(tmp_path):
    """Through train_glow.main and the shared Driver.main: the flags land in cfg['glow'] after process_control, the tag stays
    the reference's, and cglow refuses a False."""
    base = ['--data_name', 'CIFAR10', '--control_name', '0.5']
    c = _probe(base + ['--model_name', 'mcglow', '--glow_affine', 'False', '--glow_conv_lu', 'False'], tmp_path)
    assert c['glow'] == {'hidden_size': 512, 'K': 16, 'L': 3, 'affine': False, 'conv_lu': False}
    assert c['tag'] == '0_CIFAR10_label_mcglow_0.5'
    c = _probe(['--data_name', 'CIFAR10', '--control_name', 'None', '--model_name', 'cglow', '--glow_conv_lu', 'False'], tmp_path)
    assert 'Not valid invertible conv' in c['error'] and 'tag' not in c
