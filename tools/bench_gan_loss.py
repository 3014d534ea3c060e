#!/usr/bin/env python3
"""cfg['loss_type'] (train_gan.py:55,148-156,168-174) on the HIP path: ms/step of the graph-replayed GraphedGANTrainer with
the hinge loss and with BCE, for MCGAN and CGAN on CIFAR-10 at B = 128 in bf16.  The two losses are captured side by side on
models of the same seed and timed in alternating windows of one run; training simply goes on from window to window, as in a
plain `bench.py` run (no `device_restore` between replays: it bumps the codebooks' versions, and the eager image refresh
behind it would rebuild the per-mode compaction tables a captured graph still reads).  Reported per loss: the
median over the windows and their spread.  Also counts the kernel
launches of one eager iteration per loss (torch.profiler): the BCE step must not add a launch.  Writes one JSON object to
--out and prints it.
usage: tools/bench_gan_loss.py [--batch 128] [--steps 20] [--warmup 5] [--windows 7] [--dtype bfloat16] [--models mcgan,cgan]
                               [--no-launch-count] [--out profiles/gan_loss_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_cgan import _launches, _model  # noqa: E402

LOSSES = ('Hinge', 'BCE')


def _window(tr, img, lab, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        out = tr.train_iteration(img, lab)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps, out


def run(name, dtype_name, batch, steps, warmup, windows, count=True):
    from mcgen_amd.trainer import GANTrainer, GraphedGANTrainer
    r = {}
    trainers = {}
    for lt in LOSSES:
        m, shape, classes = _model(name, 'CIFAR10', dtype_name)            # (seeded: both losses start from the same weights)
        g = torch.Generator(device='cuda').manual_seed(1)
        img = torch.rand(batch, *shape, device='cuda', generator=g) * 2 - 1
        lab = torch.randint(0, classes, (batch,), device='cuda', generator=g)
        r[lt] = {}
        if count:
            eager = GANTrainer(m, classes, loss_type=lt)
            eager.train_iteration(img, lab)                                 # (first launches load code objects)
            r[lt]['launches_per_step_eager'] = _launches(lambda: eager.train_iteration(img, lab))
        tr = GraphedGANTrainer(m, classes, loss_type=lt)
        tr.capture(img, lab)
        trainers[lt] = (tr, img, lab)
    times = {lt: [] for lt in LOSSES}
    for w in range(-1, windows):                                            # window -1 warms both up and is dropped
        for lt in LOSSES:
            tr, img, lab = trainers[lt]
            ms, out = _window(tr, img, lab, warmup if w < 0 else steps)
            if w >= 0:
                times[lt].append(ms)
                r[lt].update(d_loss=float(out[0]), g_loss=float(out[1]))
    for lt in LOSSES:
        t = times[lt]
        r[lt].update(ms_per_step_median=round(statistics.median(t), 4), ms_per_step_min=round(min(t), 4),
                     ms_per_step_max=round(max(t), 4), windows=[round(x, 4) for x in t])
    h, b = r['Hinge']['ms_per_step_median'], r['BCE']['ms_per_step_median']
    r['bce_minus_hinge_ms'] = round(b - h, 4)
    r['hinge_spread_ms'] = round(r['Hinge']['ms_per_step_max'] - r['Hinge']['ms_per_step_min'], 4)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--dtype', default='bfloat16')
    ap.add_argument('--models', default='mcgan,cgan')
    ap.add_argument('--no-launch-count', action='store_true', help='skip torch.profiler (under an external profiler)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gan_loss_bench.json'))
    a = ap.parse_args()
    res = {'workload': 'gan_loss_type', 'data': 'CIFAR10', 'batch': a.batch, 'dtype': a.dtype, 'steps_per_window': a.steps,
           'windows': a.windows, 'config': '5 D + 1 G updates, Adam 2e-4 (0.5, 0.999), graph replay, losses alternating',
           'device': torch.cuda.get_device_name(0)}
    for name in a.models.split(','):
        res[name] = run(name, a.dtype, a.batch, a.steps, a.warmup, a.windows, not a.no_launch_count)
    text = json.dumps(res)
    with open(a.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
