"""cfg['loss_type'] = 'BCE' without a GPU: the float64 references of tests/gan_loss_ref.py against torch's own float64
autograd of the reference's expressions (train_gan.py:149-152,169-170), the BCE oracle, the --loss_type flag, the C ABI's
declarations and the host-side refusals of the loss-typed entry points, which return before any launch."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import gan_loss_ref as G
import golden_util as gu

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(a, b, tol=1e-13):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max())), float((a - b).abs().max())


@pytest.mark.parametrize('n', [1, 2, 11, 22, 257])
def test_bce_references_are_torch_autograd(n):
    """bce_d / bce_g against F.binary_cross_entropy_with_logits in float64 with targets of ones / zeros of shape [N, 1], as the
    reference writes them; N >= 11 holds logits 0, +-1, +-17, +-88.8, +-100.5 and +-200.  Everything is finite."""
    real, fake = G.logits_with_extremes(n, 'real'), G.logits_with_extremes(n, 'fake').flip(0)
    if n >= len(G.EXTREMES):
        for x in (real, fake):
            assert set(G.EXTREMES) <= set(float(v) for v in x.double().round(decimals=4))
    r = real.double().view(n, 1).requires_grad_(True)
    f = fake.double().view(n, 1).requires_grad_(True)
    d_loss = F.binary_cross_entropy_with_logits(r, torch.ones((n, 1), dtype=F64)) + \
        F.binary_cross_entropy_with_logits(f, torch.zeros((n, 1), dtype=F64))
    d_loss.backward()
    loss, dr, df, labs = G.bce_d(real, fake)
    _close(loss, d_loss.detach()); _close(dr, r.grad.view(-1)); _close(df, f.grad.view(-1))
    assert float(labs) == float(loss) and all(bool(torch.isfinite(t).all()) for t in (loss, dr, df))
    f2 = fake.double().view(n, 1).requires_grad_(True)
    g_loss = F.binary_cross_entropy_with_logits(f2, torch.ones((n, 1), dtype=F64))
    g_loss.backward()
    loss, df, labs = G.bce_g(fake)
    _close(loss, g_loss.detach()); _close(df, f2.grad.view(-1))
    assert float(labs) == float(loss) and bool(torch.isfinite(df).all())
    assert bool((dr <= 0).all()) and bool((df <= 0).all())


def test_bce_reference_at_the_extremes():
    """An exact 0 logit gives -+0.5 / N; at +-200 the saturated side is 0 to within a subnormal and the other -+1 / N."""
    x = torch.tensor([0.0, 200.0, -200.0])
    _, dr, df, _ = G.bce_d(x, x)
    assert float(dr[0]) == -0.5 / 3 and float(df[0]) == 0.5 / 3
    assert abs(float(dr[1])) < G.TINY and float(dr[2]) == -1.0 / 3
    assert float(df[1]) == 1.0 / 3 and abs(float(df[2])) < G.TINY
    assert float(G.softplus(torch.tensor([200.0]))) == 200.0 and 0 < float(G.softplus(torch.tensor([-200.0]))) < G.TINY


def test_bce_oracle_is_the_oracle_with_two_lines_replaced():
    """One iteration of the BCE oracle on mcgan_small.npz: its losses are what the oracle's own forwards give under the BCE
    expressions before the first update (d_iters = 1 has no earlier update), and differ from the hinge oracle's."""
    from oracle import mcgan_oracle as O
    d = gu.load_npz('mcgan_small.npz')
    sd = gu.state_from_npz(d)
    img, lab = torch.from_numpy(d['img']), torch.from_numpy(d['label'])
    zs = [torch.from_numpy(z) for z in d['z'][:2]]
    n = img.size(0)
    bce = G.OracleMCGANBCE(sd, classes=10, d_iters=1, g_iters=1)
    assert isinstance(bce, O.OracleMCGAN)
    dl, gl = bce.train_iteration(img, lab, zs)
    probe = O.OracleMCGAN(sd, classes=10, d_iters=1, g_iters=1)
    with torch.no_grad():
        d_x = probe.discriminate(img, lab)
        d_gz = probe.discriminate(probe.generate(lab, zs[0]), lab)
    ref, _, _, _ = G.bce_d(d_x.view(-1), d_gz.view(-1))
    assert abs(dl - float(ref)) < 1e-5, (dl, float(ref))
    hl = O.OracleMCGAN(sd, classes=10, d_iters=1, g_iters=1).train_iteration(img, lab, zs)
    assert abs(hl[0] - dl) > 1e-3 and abs(hl[1] - gl) > 1e-3 and gl > 0
    assert n == 8


def test_loss_type_flag():
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        import _flags
    finally:
        sys.path.pop(0)
    argv = ['train_gan.py', '--data_name', 'CIFAR10', '--loss_type', 'BCE', '--model_name', 'mcgan']
    assert _flags.pop_loss_type_flags(argv) == {'loss_type': 'BCE'}
    assert argv == ['train_gan.py', '--data_name', 'CIFAR10', '--model_name', 'mcgan']
    assert _flags.pop_loss_type_flags(['train_gan.py', '--loss_type=Hinge']) == {'loss_type': 'Hinge'}
    with pytest.raises(ValueError, match='Not valid loss type'):
        _flags.pop_loss_type_flags(['train_gan.py', '--loss_type', 'WGAN'])
    cfg = {'loss_type': 'Hinge'}                             # what the driver sets after its parser ran (train_gan.py:55)
    cfg.update(_flags.pop_loss_type_flags(['train_gan.py', '--data_name', 'CIFAR10']))
    assert cfg['loss_type'] == 'Hinge'


_DRIVER = r'''
import sys
sys.path[:0] = [ROOT + '/compat', ROOT]
class Stub:
    def __init__(self, *a, **k):
        self.a, self.k = a, k
import mcgen_amd.trainer
mcgen_amd.trainer.GraphedGANTrainer = Stub
import train_gan
from config import cfg
sys.argv = ['train_gan.py', '--data_name', 'CIFAR10', '--model_name', MODEL] + FLAGS
train_gan.parse()
cfg['classes_size'] = 10
assert cfg['loss_type'] == WANT, cfg['loss_type']
assert train_gan.make_trainer(object(), 2e-4, (0.5, 0.999)).k['loss_type'] == WANT
assert 'BCE' not in train_gan.model_tag(0) and 'Hinge' not in train_gan.model_tag(0)
print('WIRING-OK')
'''


@pytest.mark.parametrize('model', ['mcgan', 'cgan'])
@pytest.mark.parametrize('flags,want', [([], 'Hinge'), (['--loss_type', 'BCE'], 'BCE')])
def test_driver_hands_loss_type_to_the_trainer(flags, want, model):
    """compat/train_gan.py: cfg['loss_type'] is 'Hinge' unless --loss_type says otherwise, reaches make_trainer and stays out
    of the model tag (a stub stands in for the trainer class; one process per case: a driver parses its command line once)."""
    import subprocess
    code = _DRIVER.replace('ROOT', repr(ROOT)).replace('MODEL', repr(model)).replace('FLAGS', repr(flags)).replace('WANT', repr(want))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'WIRING-OK' in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_trainer_refuses_an_unknown_loss_type():
    from mcgen_amd import ops
    assert ops.gan_loss_id('Hinge') == 0 and ops.gan_loss_id('BCE') == 1
    with pytest.raises(ValueError, match='Not valid loss type'):
        ops.gan_loss_id('WGAN')


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('mcgen_gan_loss_d', 'mcgen_gan_loss_g', 'mcgen_dtail_loss_fused', 'mcgen_dtail_pair_wgrad_gan_loss')


def test_header_declares_the_loss_typed_entries():
    from mcgen_amd import _lib
    assert _lib.CONSTANTS['MCGEN_GAN_LOSS_HINGE'] == 0 and _lib.CONSTANTS['MCGEN_GAN_LOSS_BCE'] == 1
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
    # the new entries take the old ones' arguments with loss_type in front of the stream (mcgen_gan_loss_*: behind N)
    n = {k: len(_lib.SYMBOLS[k][1]) for k in _lib.SYMBOLS}
    assert n['mcgen_gan_loss_d'] == n['mcgen_hinge_d'] + 1 and n['mcgen_gan_loss_g'] == n['mcgen_hinge_g'] + 1
    assert n['mcgen_dtail_loss_fused'] == n['mcgen_dtail_hinge_fused'] + 1
    assert n['mcgen_dtail_pair_wgrad_gan_loss'] == n['mcgen_dtail_pair_wgrad_loss'] + 1


@pytest.fixture(scope='module')
def lib():
    from mcgen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


_BUF = torch.zeros(64)
P = _BUF.data_ptr()          # a non-null address: the refused calls never pass it on


def _refused(lib, rc, text):
    assert rc != 0
    assert text.encode() in lib.mcgen_last_error(), lib.mcgen_last_error()


def test_library_exports_the_loss_typed_entries(lib):
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS)


def test_gan_loss_refusals(lib):
    for lt in (2, -1):
        _refused(lib, lib.mcgen_gan_loss_d(P, P, 4, lt, P, P, P, None), f'gan_loss_d: unknown loss_type {lt}')
        _refused(lib, lib.mcgen_gan_loss_g(P, 4, lt, P, P, None), f'gan_loss_g: unknown loss_type {lt}')
    for lt in (0, 1):
        for i in (0, 1, 4, 5, 6):
            a = [P, P, 4, lt, P, P, P, None]
            a[i] = None
            _refused(lib, lib.mcgen_gan_loss_d(*a), 'gan_loss_d: null pointer')
        for i in (0, 3, 4):
            a = [P, 4, lt, P, P, None]
            a[i] = None
            _refused(lib, lib.mcgen_gan_loss_g(*a), 'gan_loss_g: null pointer')
        for n in (0, -3):
            _refused(lib, lib.mcgen_gan_loss_d(P, P, n, lt, P, P, P, None), 'gan_loss_d: N must be positive')
            _refused(lib, lib.mcgen_gan_loss_g(P, n, lt, P, P, None), 'gan_loss_g: N must be positive')


def _tail_args(n=4, hw=2, c=8, mode=1, lt=1, code=None):
    return [P, 0, code, P, P, P, P, P, P, P, n, hw, c, mode, lt, None]


def test_fused_tail_refusals(lib):
    f = lib.mcgen_dtail_loss_fused
    _refused(lib, f(*_tail_args(lt=2)), 'dtail_loss_fused: unknown loss_type 2')
    for lt in (0, 1):
        for i in (0, 3, 4, 5, 6, 7, 8, 9):                   # (code, argument 2, may be NULL: no MultimodalController)
            a = _tail_args(lt=lt)
            a[i] = None
            _refused(lib, f(*a), 'dtail_loss_fused: null pointer')
        _refused(lib, f(*_tail_args(n=0, lt=lt)), 'dtail_loss_fused: N and HW must be positive')
        _refused(lib, f(*_tail_args(n=-2, mode=0, lt=lt)), 'dtail_loss_fused: N and HW must be positive')
        _refused(lib, f(*_tail_args(n=5, mode=0, lt=lt)), 'dtail_loss_fused: mode 0 (the discriminator loss over a paired batch, N even)')
        _refused(lib, f(*_tail_args(mode=2, lt=lt)), 'dtail_loss_fused: mode 0')
        for c in (12, 2056, 0):
            _refused(lib, f(*_tail_args(c=c, lt=lt)), 'dtail_loss_fused: C must be a multiple of 8, at most 2048')


def test_pair_wgrad_gan_loss_refusals(lib):
    f = lib.mcgen_dtail_pair_wgrad_gan_loss
    args = lambda n=4, c=8, lt=1: [P, P, P, P, n, c, P, P, P, P, P, lt, None]          # noqa: E731
    _refused(lib, f(*args(lt=7)), 'dtail_pair_wgrad_gan_loss: unknown loss_type 7')
    for lt in (0, 1):
        for i in (0, 1, 2, 3, 6, 7, 8, 9, 10):
            a = args(lt=lt)
            a[i] = None
            _refused(lib, f(*a), 'dtail_pair_wgrad_gan_loss: null pointer')
        _refused(lib, f(*args(n=0, lt=lt)), 'dtail_pair_wgrad_gan_loss: N and C must be positive')
        _refused(lib, f(*args(c=0, lt=lt)), 'dtail_pair_wgrad_gan_loss: N and C must be positive')
