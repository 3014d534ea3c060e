#!/usr/bin/env python3
"""The LeCam regulariser of the discriminator loss (trainer.FusedLeCam) on the HIP path: ms/step of the
graph-replayed GraphedGANTrainer with lecam_lambda = 0 and with lecam_lambda > 0, for MCGAN and CGAN on CIFAR-10 at B = 128
in bf16.  The two settings are captured side by side on models of the same seed and timed in alternating windows of one run,
exactly as tools/bench_gan_loss.py times the two loss types (training goes on from window to window).  Reported per setting:
the median over the windows and their spread.  Also counts the kernel launches of one eager iteration per setting
(torch.profiler): the regulariser must not add a launch -- that is the acceptance condition; the step-time difference is
reported, not gated.  Writes one JSON object to --out and prints it.
usage: tools/bench_lecam.py [--batch 128] [--steps 20] [--warmup 5] [--windows 7] [--dtype bfloat16] [--models mcgan,cgan]
                            [--lecam_lambda 0.3] [--loss_type Hinge] [--no-launch-count] [--out profiles/lecam_bench.json]"""
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
from bench_gan_loss import _window  # noqa: E402


def run(name, dtype_name, batch, steps, warmup, windows, lam, loss_type, count=True):
    from mcgen_amd.trainer import GANTrainer, GraphedGANTrainer
    settings = {'off': 0.0, 'on': lam}
    r, trainers = {}, {}
    for key, value in settings.items():
        m, shape, classes = _model(name, 'CIFAR10', dtype_name)            # (seeded: both settings start from the same weights)
        g = torch.Generator(device='cuda').manual_seed(1)
        img = torch.rand(batch, *shape, device='cuda', generator=g) * 2 - 1
        lab = torch.randint(0, classes, (batch,), device='cuda', generator=g)
        r[key] = {'lecam_lambda': value}
        if count:
            eager = GANTrainer(m, classes, loss_type=loss_type, lecam_lambda=value)
            eager.train_iteration(img, lab)                                 # (first launches load code objects)
            r[key]['launches_per_step_eager'] = _launches(lambda: eager.train_iteration(img, lab))
        tr = GraphedGANTrainer(m, classes, loss_type=loss_type, lecam_lambda=value)
        tr.capture(img, lab)
        trainers[key] = (tr, img, lab)
    times = {key: [] for key in settings}
    for w in range(-1, windows):                                            # window -1 warms both up and is dropped
        for key in settings:
            tr, img, lab = trainers[key]
            ms, out = _window(tr, img, lab, warmup if w < 0 else steps)
            if w >= 0:
                times[key].append(ms)
                r[key].update(d_loss=float(out[0]), g_loss=float(out[1]))
    for key in settings:
        t = times[key]
        r[key].update(ms_per_step_median=round(statistics.median(t), 4), ms_per_step_min=round(min(t), 4),
                      ms_per_step_max=round(max(t), 4), windows=[round(x, 4) for x in t])
    lc = trainers['on'][0].lecam
    r['on'].update(a_R=float(lc.anchors()[0]), a_F=float(lc.anchors()[1]), d_updates=int(lc.step_count),
                   **{k: float(v) for k, v in lc.stats().items()})
    r['on_minus_off_ms'] = round(r['on']['ms_per_step_median'] - r['off']['ms_per_step_median'], 4)
    r['off_spread_ms'] = round(r['off']['ms_per_step_max'] - r['off']['ms_per_step_min'], 4)
    if count:
        r['launches_equal'] = r['on']['launches_per_step_eager'] == r['off']['launches_per_step_eager']
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--dtype', default='bfloat16')
    ap.add_argument('--models', default='mcgan,cgan')
    ap.add_argument('--lecam_lambda', type=float, default=0.3)
    ap.add_argument('--loss_type', default='Hinge')
    ap.add_argument('--no-launch-count', action='store_true', help='skip torch.profiler (under an external profiler)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lecam_bench.json'))
    a = ap.parse_args()
    res = {'workload': 'gan_lecam', 'data': 'CIFAR10', 'batch': a.batch, 'dtype': a.dtype, 'steps_per_window': a.steps,
           'windows': a.windows, 'loss_type': a.loss_type,
           'config': '5 D + 1 G updates, Adam 2e-4 (0.5, 0.999), graph replay, lecam_lambda 0 and > 0 alternating',
           'device': torch.cuda.get_device_name(0)}
    for name in a.models.split(','):
        res[name] = run(name, a.dtype, a.batch, a.steps, a.warmup, a.windows, a.lecam_lambda, a.loss_type, not a.no_launch_count)
    text = json.dumps(res)
    with open(a.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
