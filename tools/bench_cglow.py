#!/usr/bin/env python3
"""CGlow training step (train_glow.py:108-121) on the HIP path: ms/step of the graph-replayed GlowTrainer at B = 128 on the
config widths (hidden 512, K = 16, L = 3) for Omniglot (1x32x32, 1623 modes) and CIFAR10 (3x32x32, 10 modes), fp32 and bf16,
with MCGlow's graphed step on the same data configuration and dtype measured in the same run as the yardstick; the two
CGlow-only launches (the label-conditioned prior and its backward) timed on their own at both shapes, and the HIP-library
calls of one eager step counted.  Prints one JSON line and writes it to --out.
usage: tools/bench_cglow.py [--batch 128] [--steps 20] [--warmup 3] [--trials 5] [--dtypes float32,bfloat16] [--data Omniglot,CIFAR10]
                            [--no-mcglow] [--out profiles/cglow_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DTYPES = {'float32': torch.float32, 'bfloat16': torch.bfloat16}
DATA = {'Omniglot': (1, 1623), 'CIFAR10': (3, 10)}       # channels, modes


def _model(name, data, dtype_name):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    channels, modes = DATA[data]
    cfg.update(model_name=name, data_name=data, device='cuda', classes_size=modes, controller_rate=0.5,
               data_shape=[channels, 32, 32], compute_dtype=dtype_name)
    cfg['glow'] = {'hidden_size': 512, 'K': 16, 'L': 3, 'affine': True, 'conv_lu': True}
    torch.manual_seed(0); np.random.seed(0)
    m = getattr(models, name)().cuda()
    return m.set_compute_dtype(DTYPES[dtype_name]), channels, modes


def _time(fn, steps, warmup, trials):
    """`trials` windows of `steps` calls between device events, after `warmup` calls -> ([ms per call of each window], last
    result).  The spread of the windows is what two configurations' figures have to differ by to be told apart."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(trials):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(steps):
            out = fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e) / steps)
    return ms, out


def _stats(ms, digits=4, scale=1.0):
    ms = sorted(m * scale for m in ms)
    return {'median': round(ms[len(ms) // 2], digits), 'min': round(ms[0], digits), 'max': round(ms[-1], digits)}


def _inputs(m, channels, modes, batch):
    g = torch.Generator(device='cuda').manual_seed(1)
    img = torch.rand(batch, channels, 32, 32, device='cuda', generator=g) * 2 - 1
    lab = torch.randint(0, modes, (batch,), device='cuda', generator=g)
    m.train(True)
    with torch.no_grad():                                 # the data-dependent ActNorm initialisation (train_glow.py:60-67)
        m({'img': img, 'label': lab})
    return img, lab


def train_step(name, data, dtype_name, batch, steps, warmup, trials):
    from mcgen_amd.trainer import GlowTrainer
    m, channels, modes = _model(name, data, dtype_name)
    img, lab = _inputs(m, channels, modes, batch)
    tr = GlowTrainer(m)
    tr.capture(img, lab)
    ms, loss = _time(lambda: tr.train_iteration(img, lab), steps, warmup, trials)
    st = _stats(ms)
    return {'ms_per_step': st, 'images_per_s': round(batch / st['median'] * 1e3), 'loss': float(loss)}


def library_calls(name, data, dtype_name, batch):
    """Calls into the HIP library during one eager step (forward, backward, clip, Adam); torch's own tensor ops not counted."""
    from mcgen_amd import ops
    from mcgen_amd.trainer import GlowTrainer
    m, channels, modes = _model(name, data, dtype_name)
    img, lab = _inputs(m, channels, modes, batch)
    tr = GlowTrainer(m)
    tr.train_iteration(img, lab)
    seen, orig = [], ops.check
    ops.check = lambda rc, what='': (seen.append(what), orig(rc, what))[1]
    try:
        tr.train_iteration(img, lab)
    finally:
        ops.check = orig
    return len(seen)


def launches(data, dtype_name, batch, steps, warmup, trials):
    """us per call of the launches CGlow puts where MCGlow runs a convolution over zeros, eager, at the config shapes."""
    from mcgen_amd import ops
    dt = DTYPES[dtype_name]
    channels, modes = DATA[data]
    c2 = 32 * channels                                    # the last block's prior: 2c = 8 x its 4 x channels inputs
    g = torch.Generator(device='cuda').manual_seed(2)
    b_p, s_p, b_e, s_e = (0.1 * torch.randn(c2, device='cuda', generator=g) for _ in range(4))
    w_e = 0.1 * torch.randn(c2, modes, 1, 1, device='cuda', generator=g)
    lab = torch.randint(0, modes, (batch,), device='cuda', generator=g)
    dprior = torch.randn(batch, 4, 4, c2, device='cuda', generator=g).to(dt)
    grads = [torch.empty_like(t) for t in (b_p, s_p)] + [torch.empty(c2, c2 // 2, 3, 3, device='cuda')] + \
            [torch.empty_like(t) for t in (w_e, b_e, s_e)]
    jobs = {'prior': lambda: ops.cglow_prior(b_p, s_p, w_e, b_e, s_e, lab, 4, 4, dt),
            'prior_bwd(3 launches)': lambda: ops.cglow_prior_bwd(dprior, b_p, s_p, w_e, b_e, s_e, lab, *grads)}
    return {k: _stats(_time(fn, steps, warmup, trials)[0], 2, 1e3) for k, fn in jobs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--trials', type=int, default=5, help='timed windows of --steps replays each; median, min and max are reported')
    ap.add_argument('--dtypes', default='float32,bfloat16')
    ap.add_argument('--data', default='Omniglot,CIFAR10')
    ap.add_argument('--no-mcglow', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cglow_bench.json'))
    a = ap.parse_args()
    res = {'workload': 'cglow_train', 'batch': a.batch, 'steps': a.steps, 'warmup': a.warmup, 'trials': a.trials,
           'config': 'hidden 512, K 16, L 3, 32x32 images (1 channel with 1623 modes, 3 with 10), Adam 3e-4, clip 1, '
                     'graph-replayed step; per configuration `trials` windows of `steps` replays between device events: median, min, max',
           'device': torch.cuda.get_device_name(0)}
    names = ('cglow',) if a.no_mcglow else ('cglow', 'mcglow')
    for dt in a.dtypes.split(','):
        for data in a.data.split(','):
            for name in names:
                res[f'{name}/{data}/{dt}'] = train_step(name, data, dt, a.batch, a.steps, a.warmup, a.trials)
            res[f'launch_us/{data}/{dt}'] = launches(data, dt, a.batch, 200, 20, a.trials)
    res['library_calls_per_step'] = {n: library_calls(n, 'Omniglot', 'bfloat16', a.batch) for n in names}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
