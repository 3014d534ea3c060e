"""The LeCam regulariser without a GPU: tests/lecam_ref.py's float64 references against torch's float64 autograd of the
written-out loss, the anchor recursion over several updates, lambda = 0 against the references without the regulariser,
the oracle, the flags, the host-side refusals and the C ABI (every refusal of the three entries happens before a launch)."""
import os
import sys

import pytest
import torch

import gan_loss_ref as G
import golden_util as gu
import lecam_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
STATES = [{'a_R': 0.0, 'a_F': 0.0, 't': 0}, {'a_R': 0.3, 'a_F': -0.2, 't': 4}, {'a_R': -50.0, 'a_F': 50.0, 't': 9}]


@pytest.mark.parametrize('loss_type', ['Hinge', 'BCE'])
@pytest.mark.parametrize('n', [1, 7, 300])
def test_references_are_torch_autograd(n, loss_type):
    """loss, dreal and dfake of lecam_d are the value and the float64 autograd gradients of the written-out loss, with the
    anchors as constants; off (t < start, lambda = 0) they are the base references'."""
    real = G.logits_with_extremes(n, 'lr').clamp(-60, 60)     # (float64 autograd of relu / BCE: no overflow to guard here)
    fake = G.logits_with_extremes(n, 'lf').flip(0).clamp(-60, 60)
    for state in STATES:
        for lam, start in ((0.3, 0), (0.3, 5), (0.0, 0), (2.5, 9)):
            ref = L.lecam_d(real, fake, loss_type, state, lam, 0.99, start)
            assert ref['active'] == (lam > 0 and state['t'] >= start)
            r, f = real.to(F64).requires_grad_(True), fake.to(F64).requires_grad_(True)
            loss = L.written_out_loss(r, f, loss_type, state, lam, start)
            gr, gf = torch.autograd.grad(loss, (r, f))
            loss = float(loss.detach())
            assert abs(loss - float(ref['loss'])) <= 1e-12 * max(1.0, abs(loss))
            # (relu'(0) is 0 for autograd and for the reference's strict comparison alike)
            assert torch.allclose(gr, ref['dreal'], rtol=1e-12, atol=1e-15)
            assert torch.allclose(gf, ref['dfake'], rtol=1e-12, atol=1e-15)
            if not ref['active']:
                bl, bdr, bdf, _ = L.base_d(real, fake, loss_type)
                assert float(bl) == float(ref['loss']) and torch.equal(bdr, ref['dreal']) and torch.equal(bdf, ref['dfake'])
            for k in ('loss_tol', 'R_tol'):
                assert float(ref[k]) > 0
            # (a closed hinge with the term off is an exact 0: its bound is 0)
            assert bool((ref['dreal_tol'] >= 0).all()) and bool((ref['dfake_tol'] >= 0).all())
            if ref['active']:
                assert bool((ref['dreal_tol'] > 0).all()) and bool((ref['dfake_tol'] > 0).all())


def test_lambda_zero_is_the_base_losses_exactly():
    """lambda = 0 reproduces gan_loss_ref.bce_d and the hinge expressions exactly, whatever the anchors hold."""
    real, fake = G.logits_with_extremes(40, 'zr'), G.logits_with_extremes(40, 'zf')
    state = {'a_R': 7.0, 'a_F': -3.0, 't': 11}
    ref = L.lecam_d(real, fake, 'BCE', state, 0.0, 0.99, 0)
    bl, bdr, bdf, _ = G.bce_d(real, fake)
    assert float(ref['loss']) == float(bl) and torch.equal(ref['dreal'], bdr) and torch.equal(ref['dfake'], bdf)
    assert torch.equal(ref['dreal_tol'], G.grad_tol(bdr))
    ref = L.lecam_d(real, fake, 'Hinge', state, 0.0, 0.99, 0)
    r, f = real.to(F64), fake.to(F64)
    assert float(ref['loss']) == float(torch.relu(1 - r).sum() / 40 + torch.relu(1 + f).sum() / 40)
    assert ref['dreal'].tolist() == [(-1 / 40 if 1 - v > 0 else 0.0) for v in r.tolist()]
    assert ref['dfake'].tolist() == [(1 / 40 if 1 + v > 0 else 0.0) for v in f.tolist()]
    assert ref['state']['t'] == 12                           # the state moves all the same: the entry was called


def test_anchor_recursion():
    """Six updates from the fresh state with start = 3: update 0 copies the means, later ones average with decay; the term
    is off for t = 0, 1, 2 (the anchors move all the same) and on from t = 3; r_t counts signs with sign(0) = 0."""
    gen = torch.Generator().manual_seed(3)
    state, decay, lam, start = L.fresh_state(), 0.75, 0.5, 3
    a_r = a_f = 0.0
    for t in range(6):
        real, fake = torch.randn(5, generator=gen) + 1, torch.randn(5, generator=gen) - 1
        real[0] = 0.0
        ref = L.lecam_d(real, fake, 'Hinge', state, lam, decay, start)
        assert ref['active'] == (t >= start)
        base = L.base_d(real, fake, 'Hinge')[0]
        want = base + (lam * (((real.double() - a_f) ** 2).mean() + ((fake.double() - a_r) ** 2).mean()) if t >= start else 0.0)
        assert abs(float(ref['loss']) - float(want)) < 1e-12
        m_r, m_f = float(real.double().mean()), float(fake.double().mean())
        a_r, a_f = (m_r, m_f) if t == 0 else (decay * a_r + (1 - decay) * m_r, decay * a_f + (1 - decay) * m_f)
        a_r, a_f = L.f32(a_r), L.f32(a_f)                    # (the kernels keep the anchors in fp32: so does the next update)
        state = ref['state']
        assert state['t'] == t + 1
        assert abs(state['a_R'] - a_r) < 1e-6 and abs(state['a_F'] - a_f) < 1e-6
        state = dict(state, a_R=a_r, a_F=a_f)
        signs = sum((v > 0) - (v < 0) for v in real.tolist())
        assert float(ref['stats']['r_t']) == signs / 5 and abs(float(ref['stats']['m_R']) - m_r) < 1e-15


def test_oracle_with_lambda_zero_is_the_oracle_and_the_term_changes_it():
    from oracle import mcgan_oracle as O
    d = gu.load_npz('mcgan_small.npz')
    sd = gu.state_from_npz(d)
    img, lab = torch.from_numpy(d['img']), torch.from_numpy(d['label'])
    zs = [torch.from_numpy(z) for z in d['z'][:6]]
    plain = O.OracleMCGAN(sd, classes=10).train_iteration(img, lab, zs)
    off = L.OracleMCGANLeCam(sd, 10, 0.0, decay=0.9)
    assert off.train_iteration(img, lab, zs) == plain
    assert off.lecam['t'] == 5 and off.lecam['a_R'] != 0.0
    on = L.OracleMCGANLeCam(sd, 10, 0.3, decay=0.9)
    got = on.train_iteration(img, lab, zs)
    assert abs(got[0] - plain[0]) > 1e-4 and on.lecam['t'] == 5
    late = L.OracleMCGANLeCam(sd, 10, 0.3, decay=0.9, start=5)
    assert late.train_iteration(img, lab, zs) == plain       # (five updates, all before start)
    assert late.lecam == off.lecam                           # the anchors moved all the same, along the plain trajectory


# ---- flags and host-side refusals ------------------------------------------------------------------------------------
def _flags():
    sys.path.insert(0, os.path.join(ROOT, 'compat'))
    try:
        import _flags
    finally:
        sys.path.pop(0)
    return _flags


def test_lecam_flags():
    f = _flags()
    argv = ['train_gan.py', '--data_name', 'CIFAR10', '--lecam_lambda', '0.3', '--lecam_start=40', '--lecam_decay', '0.9']
    assert f.pop_lecam_flags(argv) == {'lecam_lambda': 0.3, 'lecam_decay': 0.9, 'lecam_start': 40}
    assert argv == ['train_gan.py', '--data_name', 'CIFAR10']
    assert f.pop_lecam_flags(['train_gan.py']) == {'lecam_lambda': 0.0, 'lecam_decay': 0.99, 'lecam_start': 0}
    assert f.pop_lecam_flags(['x', '--lecam_lambda', '1'])['lecam_decay'] == 0.99
    for bad in (['--lecam_lambda', '-0.1'], ['--lecam_lambda', 'inf'], ['--lecam_lambda', 'nan'],
                ['--lecam_lambda', '0.3', '--lecam_decay', '1.0'], ['--lecam_lambda', '0.3', '--lecam_decay', '-0.5'],
                ['--lecam_lambda', '0.3', '--lecam_start', '-1'], ['--lecam_decay', '0.9'], ['--lecam_start', '3']):
        with pytest.raises(ValueError, match='Not valid --lecam'):
            f.pop_lecam_flags(['train_gan.py'] + bad)


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
extra = train_gan.parse()
cfg['classes_size'] = 10
lecam = {k: extra[k] for k in ('lecam_lambda', 'lecam_decay', 'lecam_start')} if extra['lecam_lambda'] else None
k = train_gan.make_trainer(object(), 2e-4, (0.5, 0.999), lecam=lecam).k
print('WIRING', sorted((n, v) for n, v in k.items() if n.startswith('lecam')))
'''


@pytest.mark.parametrize('model', ['mcgan', 'cgan'])
def test_driver_hands_the_flags_to_the_trainer(model):
    """compat/train_gan.py: the three flags reach make_trainer; with none given the trainer is built with exactly the
    arguments it was built with before (a stub stands in for the trainer class; one process per case)."""
    import subprocess
    for flags, want in (([], '[]'),
                        (['--lecam_lambda', '0.3', '--lecam_start', '7'],
                         "[('lecam_decay', 0.99), ('lecam_lambda', 0.3), ('lecam_start', 7)]")):
        code = _DRIVER.replace('ROOT', repr(ROOT)).replace('MODEL', repr(model)).replace('FLAGS', repr(flags))
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and 'WIRING ' + want in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_trainer_refuses_bad_hyper_parameters_and_more_than_one_rank():
    """The constructor checks the LeCam arguments first, before it looks at the model or a device (a bare object stands in)."""
    from mcgen_amd.trainer import FusedLeCam, GANTrainer, GraphedGANTrainer
    for cls in (GANTrainer, GraphedGANTrainer):
        with pytest.raises(ValueError, match='lecam_lambda > 0 runs on one GPU'):
            cls(object(), 10, lecam_lambda=0.3, world_size=2)
        for kw in ({'lecam_lambda': -1.0}, {'lecam_lambda': float('nan')}, {'lecam_lambda': 0.3, 'lecam_decay': 1.0},
                   {'lecam_lambda': 0.3, 'lecam_start': -2}):
            with pytest.raises(ValueError, match='Not valid LeCam regulariser'):
                cls(object(), 10, **kw)
    assert FusedLeCam.check_hyper(0.3, 0.99, 0) == (0.3, 0.99, 0)


def test_holder_on_the_cpu(capsys):
    """FusedLeCam launches nothing: its views, hyper key and state_dict round trip work on CPU tensors."""
    from mcgen_amd import ops
    from mcgen_amd.trainer import FusedLeCam
    words, floats, t_at = ops.lecam_state_layout()
    assert words == 4 and t_at == 3 and floats == {'a_real': 0, 'a_fake': 1, 'm_real': 2, 'm_fake': 3, 'r_t': 4, 'reg': 5}
    h = FusedLeCam('cpu', 0.3, 0.9, 5)
    assert h.hyper() == (0.3, 0.9, 5) and int(h.step_count) == 0 and [float(a) for a in h.anchors()] == [0.0, 0.0]
    assert [t.data_ptr() for t in h.state_tensors()] == [h.state.data_ptr()]
    h.load_state_dict({'a_R': 0.25, 'a_F': -0.5, 'step': 17, 'stats': {'m_R': 1.0, 'm_F': -1.0, 'r_t': 0.5, 'R': 2.0}})
    sd = h.state_dict()
    assert (sd['a_R'], sd['a_F'], sd['step'], sd['lambda'], sd['decay'], sd['start']) == (0.25, -0.5, 17, 0.3, 0.9, 5)
    assert sd['stats'] == {'m_R': 1.0, 'm_F': -1.0, 'r_t': 0.5, 'R': 2.0}
    other = FusedLeCam('cpu', 0.3)
    other.load_state_dict(sd)
    assert 'LeCam state was accumulated with (lambda, decay, start) = (0.3, 0.9, 5)' in capsys.readouterr().out
    FusedLeCam('cpu', 0.3, 0.9, 5).load_state_dict(sd)
    assert capsys.readouterr().out == ''                     # (the same settings: no line)
    assert torch.equal(other.state, h.state) and other.hyper() == (0.3, 0.99, 0)     # the hyper-parameters stay the run's
    other.reset()
    assert int(other.step_count) == 0 and float(other.anchors()[0]) == 0.0


def test_checkpoint_key(tmp_path):
    """make_checkpoint / resume: the 'lecam' key is there only with a holder; a file without it resumes with fresh state
    and says so."""
    from mcgen_amd.checkpoint import make_checkpoint, resume, save
    from mcgen_amd.trainer import FusedLeCam
    model = torch.nn.Linear(2, 2)
    h = FusedLeCam('cpu', 0.3)
    h.load_state_dict({'a_R': 0.25, 'a_F': -0.5, 'step': 3})
    with_key, without = make_checkpoint(model, {}, 2, {}, lecam=h), make_checkpoint(model, {}, 2, {})
    assert set(with_key) == set(without) | {'lecam'} and with_key['lecam']['a_R'] == 0.25
    save(with_key, str(tmp_path / 'a.pt')); save(without, str(tmp_path / 'b.pt'))
    h2 = FusedLeCam('cpu', 0.3)
    resume(str(tmp_path / 'a.pt'), model, lecam=h2)
    assert torch.equal(h2.state, h.state)


def test_checkpoint_without_the_key_resumes_fresh(tmp_path, capsys):
    from mcgen_amd.checkpoint import make_checkpoint, resume, save
    from mcgen_amd.trainer import FusedLeCam
    model = torch.nn.Linear(2, 2)
    save(make_checkpoint(model, {}, 2, {}), str(tmp_path / 'b.pt'))
    h = FusedLeCam('cpu', 0.3)
    h.load_state_dict({'a_R': 0.25, 'a_F': -0.5, 'step': 3})
    resume(str(tmp_path / 'b.pt'), model, lecam=h)
    assert int(h.step_count) == 0 and float(h.anchors()[0]) == 0.0
    assert 'No LeCam state' in capsys.readouterr().out


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('mcgen_lecam_loss_d', 'mcgen_dtail_lecam_fused', 'mcgen_dtail_pair_wgrad_lecam_loss')


def test_header_declares_the_entries_and_the_state():
    import ctypes
    from mcgen_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
    st = _lib.LecamState
    assert ctypes.sizeof(st) == 32 and st.t.offset == 24 and [f for f, _ in st._fields_][:2] == ['a_real', 'a_fake']
    n = {k: len(_lib.SYMBOLS[k][1]) for k in _lib.SYMBOLS}
    assert n['mcgen_lecam_loss_d'] == n['mcgen_gan_loss_d'] + 4                  # state, lambda, decay, start
    assert n['mcgen_dtail_lecam_fused'] == n['mcgen_dtail_loss_fused'] - 1 + 3   # no mode; state, lambda, start
    assert n['mcgen_dtail_pair_wgrad_lecam_loss'] == n['mcgen_dtail_pair_wgrad_gan_loss'] + 4
    # no existing signature changed
    assert n['mcgen_dtail_loss_fused'] == 16 and n['mcgen_dtail_pair_wgrad_gan_loss'] == 13 and n['mcgen_gan_loss_d'] == 8


@pytest.fixture(scope='module')
def lib():
    from mcgen_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


_BUF = torch.zeros(64)
P = _BUF.data_ptr()          # a non-null address: the refused calls never pass it on
NAN, INF = float('nan'), float('inf')


def _refused(lib, rc, text):
    assert rc != 0
    assert text.encode() in lib.mcgen_last_error(), lib.mcgen_last_error()


def test_library_exports_the_entries(lib):
    assert all(hasattr(lib, name) for name in NEW_SYMBOLS)


def test_lecam_loss_d_refusals(lib):
    f = lib.mcgen_lecam_loss_d
    args = lambda n=4, lt=1, st=P, lam=0.3, decay=0.99, start=0: [P, P, n, lt, st, lam, decay, start, P, P, P, None]   # noqa: E731
    _refused(lib, f(*args(lt=2)), 'lecam_loss_d: unknown loss_type 2')
    for lt in (0, 1):
        for i in (0, 1, 8, 9, 10):
            a = args(lt=lt)
            a[i] = None
            _refused(lib, f(*a), 'lecam_loss_d: null pointer')
        _refused(lib, f(*args(n=0, lt=lt)), 'lecam_loss_d: N must be positive')
        _refused(lib, f(*args(st=None, lt=lt)), 'lecam_loss_d: null state')
        for lam in (-0.5, NAN, INF):
            _refused(lib, f(*args(lam=lam, lt=lt)), 'lecam_loss_d: lambda must be finite and not negative')
        for decay in (1.0, -0.1, 1.5, NAN):
            _refused(lib, f(*args(decay=decay, lt=lt)), 'lecam_loss_d: decay in [0, 1)')
        _refused(lib, f(*args(start=-1, lt=lt)), 'lecam_loss_d: start must not be negative')


def test_lecam_fused_tail_refusals(lib):
    f = lib.mcgen_dtail_lecam_fused
    args = lambda n=4, hw=2, c=8, lt=1, st=P, lam=0.3, start=0: [P, 0, None, P, P, P, P, P, P, P, n, hw, c, lt, st, lam, start, None]   # noqa: E731
    _refused(lib, f(*args(lt=3)), 'dtail_lecam_fused: unknown loss_type 3')
    for lt in (0, 1):
        for i in (0, 3, 4, 5, 6, 7, 8, 9):
            a = args(lt=lt)
            a[i] = None
            _refused(lib, f(*a), 'dtail_lecam_fused: null pointer')
        for n in (0, -2, 5):
            _refused(lib, f(*args(n=n, lt=lt)), 'dtail_lecam_fused: a paired batch (N even and positive)')
        _refused(lib, f(*args(hw=0, lt=lt)), 'dtail_lecam_fused: a paired batch')
        for c in (12, 2056, 0):
            _refused(lib, f(*args(c=c, lt=lt)), 'dtail_lecam_fused: C must be a multiple of 8, at most 2048')
        _refused(lib, f(*args(st=None, lt=lt)), 'dtail_lecam_fused: null state')
        for lam in (-0.5, NAN, INF):
            _refused(lib, f(*args(lam=lam, lt=lt)), 'dtail_lecam_fused: lambda must be finite and not negative')
        _refused(lib, f(*args(start=-1, lt=lt)), 'dtail_lecam_fused: start must not be negative')


def test_pair_wgrad_lecam_loss_refusals(lib):
    f = lib.mcgen_dtail_pair_wgrad_lecam_loss
    args = lambda n=4, c=8, lt=1, st=P, lam=0.3, decay=0.99, start=0: [P, P, P, P, n, c, P, P, P, P, P, lt, st, lam, decay, start, None]   # noqa: E731
    _refused(lib, f(*args(lt=7)), 'dtail_pair_wgrad_lecam_loss: unknown loss_type 7')
    for lt in (0, 1):
        for i in (0, 1, 2, 3, 6, 7, 8, 9, 10):
            a = args(lt=lt)
            a[i] = None
            _refused(lib, f(*a), 'dtail_pair_wgrad_lecam_loss: null pointer')
        _refused(lib, f(*args(n=0, lt=lt)), 'dtail_pair_wgrad_lecam_loss: N and C must be positive')
        _refused(lib, f(*args(c=0, lt=lt)), 'dtail_pair_wgrad_lecam_loss: N and C must be positive')
        _refused(lib, f(*args(st=None, lt=lt)), 'dtail_pair_wgrad_lecam_loss: null state')
        _refused(lib, f(*args(lam=-1.0, lt=lt)), 'dtail_pair_wgrad_lecam_loss: lambda must be finite and not negative')
        for decay in (1.0, -0.1):
            _refused(lib, f(*args(decay=decay, lt=lt)), 'dtail_pair_wgrad_lecam_loss: decay in [0, 1)')
        _refused(lib, f(*args(start=-3, lt=lt)), 'dtail_pair_wgrad_lecam_loss: start must not be negative')
