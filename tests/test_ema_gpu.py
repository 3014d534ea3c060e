"""The averaged generator on the GPU: mcgen_ema_update and mcgen_swap_f32 against float64 / bit patterns over sizes and
misaligned bases, trainer.FusedEMA inside GANTrainer (eager, graph replay, off), the weight images after a swap, and the
train_gan / generate drivers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [1, 3, 4, 255, 256, 257, 1024 * 4 + 3, 65536 + 5]
# (element offset of the first range, of the second) from a 16-byte aligned base: the four misalignments the issue's sweep
# names, on both ranges alike (vector body behind a scalar head), and two pairs that disagree (no vector body at all)
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (1, 3), (0, 2)]
GUARD = 12345.0
U = 2.0 ** -24


def _range(n, off, seed, special=True):
    """-> (whole buffer, the n-element range at element 4 + off): guard values around it, normal draws inside and, where
    there is room, a few entries of magnitude 1e-30 and 1e30."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.randn(n, generator=g)
    if special and n >= 4:
        idx = torch.randperm(n, generator=g)[:4]
        vals[idx] = torch.tensor([1e-30, -1e30, 1e30, -1e-30])
    buf = torch.full((n + 16,), GUARD)
    buf[4 + off:4 + off + n] = vals
    buf = buf.cuda()
    return buf, buf[4 + off:4 + off + n]


def _guards_ok(buf, n, off):
    b = buf.cpu()
    return bool((b[:4 + off] == GUARD).all() and (b[4 + off + n:] == GUARD).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize('n', SIZES)
def test_ema_update_against_float64(n):
    from mcgen_amd import ops
    for d in (0.5, 0.999):
        d32 = np.float32(d)
        omd32 = np.float32(1) - d32
        for oe, op_ in OFFSETS:
            ebuf, e = _range(n, oe, 10 * n + oe)
            pbuf, p = _range(n, op_, 10 * n + 5 + op_)
            e0, p0 = e.cpu().double(), p.cpu().double()
            step = torch.tensor([3, 0], dtype=torch.int64, device='cuda')
            # past the warm-up: one averaging step, the count untouched without `advance`
            ops.ema_update(e, p, step, d, start=3, advance=False)
            ref = float(d32) * e0 + float(omd32) * p0
            err = (e.cpu().double() - ref).abs()
            bound = 4 * U * torch.maximum(e0.abs(), p0.abs())
            print(f'n={n} d={d} off=({oe},{op_}): max err / bound = {float((err / bound).max()):.3f}')
            assert bool((err <= bound).all()), (n, d, oe, op_, float((err / bound).max()))
            assert torch.equal(_bits(p), _bits(p0.float())) and _guards_ok(ebuf, n, oe) and _guards_ok(pbuf, n, op_)
            assert step.tolist() == [3, 0]
            # inside the warm-up (step < start): a bit-exact copy; `advance` moves the count by exactly one
            ops.ema_update(e, p, step, d, start=4, advance=True)
            assert torch.equal(_bits(e), _bits(p)) and _guards_ok(ebuf, n, oe) and _guards_ok(pbuf, n, op_)
            assert step.tolist() == [4, 0]


def test_ema_counter_advances_once_per_update():
    """An update that takes two launches (parameters, then statistics) passes `advance` on the last one only: both see the
    same count, and it moves by one per update -- here across the warm-up's end."""
    from mcgen_amd import ops
    _, pa = _range(70001, 0, 1, special=False)
    _, pb = _range(37, 1, 2, special=False)
    ea, eb = torch.zeros_like(pa), torch.zeros_like(pb)
    step = torch.zeros(2, dtype=torch.int64, device='cuda')
    for k in range(4):
        before = (ea.clone(), eb.clone())
        ops.ema_update(ea, pa, step, 0.5, start=2, advance=False)
        ops.ema_update(eb, pb, step, 0.5, start=2, advance=True)
        assert step.tolist() == [k + 1, 0]
        for e, p, b in ((ea, pa, before[0]), (eb, pb, before[1])):
            if k < 2:
                assert torch.equal(_bits(e), _bits(p))
            else:                                        # 0.5 * (b + p): exact products, one rounding
                assert torch.equal(e.cpu(), (0.5 * b.cpu().double() + 0.5 * p.cpu().double()).float())
        pa.add_(1.0); pb.add_(1.0)


@pytest.mark.parametrize('n', SIZES)
def test_swap_bit_exact(n):
    from mcgen_amd import ops
    for oa, ob in OFFSETS:
        abuf, a = _range(n, oa, 20 * n + oa)
        bbuf, b = _range(n, ob, 20 * n + 7 + ob)
        if n >= 2:                                       # a NaN payload and a negative zero must cross unchanged too
            a.view(torch.int32)[0] = 0x7FC12345
            b.view(torch.int32)[n - 1] = -0x80000000
        a0, b0 = _bits(a), _bits(b)
        ops.swap_(a, b)
        assert torch.equal(_bits(a), b0) and torch.equal(_bits(b), a0), (n, oa, ob)
        assert _guards_ok(abuf, n, oa) and _guards_ok(bbuf, n, ob)
        ops.swap_(a, b)
        assert torch.equal(_bits(a), a0) and torch.equal(_bits(b), b0), (n, oa, ob)
        assert _guards_ok(abuf, n, oa) and _guards_ok(bbuf, n, ob)


# ---- the trainer on the small models ------------------------------------------------------------------------------------
N, ITERS = 16, 4


def _build(kind='mcgan', sd=None):
    from mcgen_amd import models
    from mcgen_amd.config import cfg, process_control
    cfg['data_name'], cfg['model_name'], cfg['device'] = 'CIFAR10', kind, 'cuda'
    cfg.pop('classes_size', None)
    process_control()
    cfg['classes_size'] = 10
    cfg['gan']['generator_hidden_size'], cfg['gan']['discriminator_hidden_size'] = [32] * 4, [16] * 4
    m = getattr(models, kind)()
    if sd is not None:
        m.load_state_dict(sd)
    return m.cuda().set_compute_dtype(torch.float32)


def _inputs():
    g = torch.Generator().manual_seed(77)
    img = (torch.rand(N, 3, 32, 32, generator=g) * 2 - 1).cuda()
    lab = torch.randint(0, 10, (N,), generator=g)
    lab[0], lab[1] = 0, 9
    zs = [torch.randn(N, 128, generator=g).cuda() for _ in range(6 * ITERS)]
    return img, lab.cuda(), zs


def _initial(kind):
    if kind == 'mcgan':
        return gu.state_from_npz(gu.load_npz('mcgan_small.npz'))
    torch.manual_seed(5)
    return {k: v.detach().cpu().clone() for k, v in _build('cgan').state_dict().items()}


def _gen_state(m):
    return {k: v.detach().cpu().clone() for k, v in m.generator.state_dict().items()}


def _run(kind, sd0, graphed=False, iters=3, visit=None, **ema):
    """`iters` iterations from `sd0` with the injected latents; -> dict(trainer, model, losses, snaps: the generator's
    state_dict after every iteration, i.e. after every generator step).  `visit(k, tr, model)` runs after iteration k."""
    from mcgen_amd.trainer import GANTrainer, GraphedGANTrainer
    img, lab, zs = _inputs()
    m = _build(kind, sd0)
    tr = (GraphedGANTrainer if graphed else GANTrainer)(m, 10, **ema)
    out = {'tr': tr, 'm': m, 'losses': [], 'snaps': []}
    if graphed:
        tr.capture(img, lab, warmup=1)
        torch.cuda.synchronize()
        out['after_capture'] = (_gen_state(m), tr.ema.state_dict() if tr.ema is not None else None)
    for k in range(iters):
        dl, gl = tr.train_iteration(img, lab, zs[6 * k:6 * k + 6])
        out['losses'].append((float(dl), float(gl)))
        out['snaps'].append(_gen_state(m))
        if visit is not None:
            visit(k, tr, m)
    out['final'] = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    out['ema'] = tr.ema.state_dict() if tr.ema is not None else None
    return out


_CACHE = {}


def _eager(kind):
    """The eager run with averaging on (decay 0.5, warm-up 1), computed once per model and shared."""
    if kind not in _CACHE:
        sd0 = _initial(kind)
        _CACHE[kind] = (sd0, _run(kind, sd0, ema_decay=0.5, ema_start=1))
    return _CACHE[kind]


def _same(a, b):
    """Equal bit for bit (float32 compared as words, so a NaN or a signed zero cannot hide a difference)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


@pytest.mark.parametrize('kind', ['mcgan', 'cgan'])
def test_trainer_eager_matches_float64_recurrence(kind):
    sd0, r = _eager(kind)
    ema, snaps = r['ema'], r['snaps']
    assert ema['step'] == 3 and (ema['decay'], ema['start']) == (0.5, 1)
    gen = r['m'].generator
    assert list(ema['params']) == [k for k, _ in gen.named_parameters()]
    assert ema['buffers'] and all(k.endswith(('running_mean', 'running_var')) for k in ema['buffers'])
    assert set(ema['buffers']) == {k for k, b in gen.named_buffers() if k.endswith(('running_mean', 'running_var'))}
    worst = 0.0
    for k, got in list(ema['params'].items()) + list(ema['buffers'].items()):
        s = [sn[k].double() for sn in snaps]
        ref = s[0]                                       # the first update is inside the warm-up: a copy
        for p in s[1:]:
            ref = 0.5 * ref + 0.5 * p
        bound = 8 * U * torch.stack([x.abs() for x in s]).max(0).values
        err = (got.cpu().double() - ref).abs()
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all()), (k, float(err.max()))
    print(f'{kind}: worst err / bound = {worst:.3f}')
    assert any(not torch.equal(snaps[0][k], snaps[2][k]) for k in ema['params'])      # (the generator did move)
    # the first update alone: an exact copy of the parameters behind the first generator step
    one = _run(kind, sd0, iters=1, ema_decay=0.5, ema_start=1)
    assert one['ema']['step'] == 1
    for k, got in list(one['ema']['params'].items()) + list(one['ema']['buffers'].items()):
        assert _same(got, one['snaps'][0][k]), k


def test_trainer_graph_replay_matches_eager_bitwise():
    sd0, e = _eager('mcgan')
    g = _run('mcgan', sd0, graphed=True, ema_decay=0.5, ema_start=1)
    gen0, ema0 = g['after_capture']
    assert ema0['step'] == 0                             # the capture warm-up advanced nothing
    for k, v in list(ema0['params'].items()) + list(ema0['buffers'].items()):
        assert _same(v, sd0['generator.' + k]), k
    for k, v in gen0.items():
        assert _same(v, sd0['generator.' + k]), k
    assert g['ema']['step'] == 3
    for kind in ('params', 'buffers'):
        for k, v in e['ema'][kind].items():
            assert _same(g['ema'][kind][k], v), k
    assert g['losses'] == e['losses']


def test_off_means_off():
    from mcgen_amd import ops
    sd0, on = _eager('mcgan')
    calls = []
    real = ops.ema_update
    ops.ema_update = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        zero = _run('mcgan', sd0, ema_decay=0.0)
        none = _run('mcgan', sd0)
    finally:
        ops.ema_update = real
    assert not calls                                     # no launch added
    for r in (zero, none):
        assert getattr(r['tr'], 'ema', None) is None
        with pytest.raises(ValueError):
            r['tr'].ema_weights()
    assert zero['losses'] == none['losses'] and list(zero['final']) == list(none['final'])
    for k, v in none['final'].items():
        assert _same(zero['final'][k], v), k
    # and with averaging on the live run is the same run: the average never feeds back
    assert on['losses'] == none['losses']
    for k, v in none['final'].items():
        assert _same(on['final'][k], v), k


def test_continuation_after_swap():
    """The weight-image hazard: an eval-mode forward on the averaged weights between two graph replays must leave no
    trace -- the live weights' images are rebuilt when the context exits, not by the next replay."""
    sd0 = _initial('mcgan')
    a = _run('mcgan', sd0, graphed=True, iters=ITERS, ema_decay=0.5, ema_start=1)
    img, lab, zs = _inputs()
    seen = {}

    def visit(k, tr, m):
        if k != 1:
            return
        before = {n: v.detach().clone() for n, v in m.state_dict().items()}
        avg = tr.ema.state_dict()
        with tr.ema_weights():
            m.train(False)
            with torch.no_grad():
                seen['inside'] = m.generate(lab, zs[0]).detach().clone()
            for kind in ('params', 'buffers'):               # the live tensors hold the averaged values
                for n, v in avg[kind].items():
                    assert _same(m.generator.state_dict()[n], v), n
        m.train(True)
        for n, v in m.state_dict().items():
            assert _same(v, before[n]), n
        for kind in ('params', 'buffers'):
            for n, v in tr.ema.state_dict()[kind].items():
                assert _same(v, avg[kind][n]), n
        seen['avg'], seen['live'] = avg, before

    b = _run('mcgan', sd0, graphed=True, iters=ITERS, visit=visit, ema_decay=0.5, ema_start=1)
    assert b['losses'] == a['losses']
    for k, v in a['final'].items():
        assert _same(b['final'][k], v), k
    assert b['ema']['step'] == a['ema']['step'] == ITERS
    for kind in ('params', 'buffers'):
        for k, v in a['ema'][kind].items():
            assert _same(b['ema'][kind][k], v), k
    # inside the context the model IS the averaged generator: a fresh model loaded with the averaged values generates the
    # same images (the same kernels on the same weights and shapes: bit for bit)
    from mcgen_amd.checkpoint import overlay_averaged_generator
    sd = {k: v.cpu() for k, v in seen['live'].items()}
    gen_sd = overlay_averaged_generator({k[len('generator.'):]: v for k, v in sd.items() if k.startswith('generator.')},
                                        {'generator_ema': {k: ({n: t.cpu() for n, t in v.items()} if isinstance(v, dict) else v)
                                                           for k, v in seen['avg'].items()}})
    fresh = _build('mcgan', sd)
    fresh.generator.load_state_dict(gen_sd)
    fresh.train(False)
    with torch.no_grad():
        ref = fresh.generate(lab, zs[0])
    assert torch.equal(seen['inside'], ref)
    live = _build('mcgan', sd)
    live.train(False)
    with torch.no_grad():
        assert not torch.equal(live.generate(lab, zs[0]), ref)       # (and the average is not the live generator)


# ---- the drivers --------------------------------------------------------------------------------------------------------
def _drv(name, args, cwd, ok=True):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'compat', name), '--data_name', 'CIFAR10', '--model_name', 'mcgan',
                        '--control_name', '0.5'] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stdout[-2000:] + r.stderr[-3000:]
    return r


def test_drivers_checkpoint_resume_and_use_ema(tmp_path):
    from mcgen_amd.checkpoint import load, resume
    from mcgen_amd.trainer import GANTrainer
    tag = '0_CIFAR10_label_mcgan_0.5'
    on, off = tmp_path / 'on', tmp_path / 'off'
    on.mkdir(); off.mkdir()
    train = ['--num_epochs', '1', '--generate_per_mode', '1', '--output_dir', './output']
    _drv('train_gan.py', train + ['--synthetic_size', '256', '--ema_decay', '0.9'], on)
    path = on / 'output' / 'model' / f'{tag}_checkpoint.pt'
    ck = load(str(path))
    assert ck['generator_ema']['step'] == 2              # 256 images, batch 128: two generator updates
    assert (ck['generator_ema']['decay'], ck['generator_ema']['start']) == (0.9, 0)
    assert set(ck) == {'cfg', 'epoch', 'model_dict', 'optimizer_dict', 'scheduler_dict', 'logger', 'generator_ema'}
    moved = [k for k, v in ck['generator_ema']['params'].items() if not torch.equal(v, ck['model_dict']['generator.' + k])]
    assert moved                                         # model_dict keeps the live weights, not the average
    # what --resume_mode 1 calls: the average comes back bit for bit (into a trainer built with other values)
    from mcgen_amd import models
    from mcgen_amd.config import cfg, process_control
    cfg.update(data_name='CIFAR10', model_name='mcgan', device='cuda')
    cfg.pop('classes_size', None); process_control()
    m = models.mcgan().cuda()
    tr = GANTrainer(m, 10, ema_decay=0.5, ema_start=7)
    resume(str(path), m, {'generator': tr.opt_g, 'discriminator': tr.opt_d}, ema=tr.ema)
    back = tr.ema.state_dict()
    assert (back['decay'], back['start'], back['step']) == (0.9, 0, 2)
    for kind in ('params', 'buffers'):
        assert list(back[kind]) == list(ck['generator_ema'][kind])
        for k, v in ck['generator_ema'][kind].items():
            assert _same(back[kind][k], v), k
    r = _drv('train_gan.py', train + ['--synthetic_size', '256', '--ema_decay', '0.9', '--resume_mode', '1'], on)
    assert 'Resume from 2' in r.stdout
    # generate.py reads <tag>_best.pt (CIFAR-10's stand-in metric keeps no best epoch: the last checkpoint stands in)
    shutil.copy(path, on / 'output' / 'model' / f'{tag}_best.pt')
    gen = ['--generate_per_mode', '2', '--save_npy', 'True', '--save_img', 'False']
    npy = on / 'output' / 'npy' / f'generated_{tag}.npy'
    _drv('generate.py', gen, on)
    plain = np.load(npy)
    _drv('generate.py', gen + ['--use_ema', 'True'], on)
    averaged = np.load(npy)
    assert plain.shape == averaged.shape == (20, 3, 32, 32) and np.isfinite(averaged).all()
    assert not np.array_equal(plain, averaged)
    # trained without averaging: today's keys, and --use_ema has nothing to load
    _drv('train_gan.py', train + ['--synthetic_size', '128', '--ema_decay', '0'], off)
    path0 = off / 'output' / 'model' / f'{tag}_checkpoint.pt'
    assert set(load(str(path0))) == {'cfg', 'epoch', 'model_dict', 'optimizer_dict', 'scheduler_dict', 'logger'}
    shutil.copy(path0, off / 'output' / 'model' / f'{tag}_best.pt')
    r = _drv('generate.py', gen + ['--use_ema', 'True'], off, ok=False)
    assert 'ValueError: Not valid checkpoint: no averaged generator (train with --ema_decay)' in r.stderr
