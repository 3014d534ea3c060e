#!/usr/bin/env python3
"""CGAN training step (train_gan.py:139-176, 5 D + 1 G updates) on the HIP path: ms/step of the graph-replayed
GraphedGANTrainer at B = 128 for CIFAR10 ([3,32,32], 10 modes, G [256]*4 / D [128]*4) and Omniglot ([1,32,32], 1623 modes,
G [512,256,128,64] / D [64,128,256,512]), fp32 and bf16, with MCGAN's graphed step on the same data set and dtype as the
yardstick.  Also reports the kernel launches of one eager CGAN step (torch.profiler).  Prints one JSON line.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel split (profiles/cgan_kernel_stats.csv).
usage: tools/bench_cgan.py [--batch 128] [--steps 30] [--warmup 5] [--dtypes float32,bfloat16] [--data CIFAR10,Omniglot]
                           [--no-mcgan] [--no-launch-count]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _model(name, data, dtype_name):
    from mcgen_amd import models
    from mcgen_amd.config import cfg, process_control
    cfg.update(data_name=data, model_name=name, device='cuda', compute_dtype=dtype_name)
    cfg['control'] = {'controller_rate': '0.5'}
    cfg.pop('classes_size', None)
    process_control()
    torch.manual_seed(0)
    m = getattr(models, name)().cuda()
    m.set_compute_dtype({'float32': torch.float32, 'bfloat16': torch.bfloat16}[dtype_name])
    return m, cfg['data_shape'], cfg['classes_size']


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps, out


def _launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:                                                          # noqa: BLE001
        return None


def run(name, data, dtype_name, batch, steps, warmup, count=True):
    from mcgen_amd.trainer import GANTrainer, GraphedGANTrainer
    m, shape, classes = _model(name, data, dtype_name)
    g = torch.Generator(device='cuda').manual_seed(1)
    img = torch.rand(batch, *shape, device='cuda', generator=g) * 2 - 1
    lab = torch.randint(0, classes, (batch,), device='cuda', generator=g)
    r = {}
    if count:
        eager = GANTrainer(m, classes)
        r['launches_per_step_eager'] = _launches(lambda: eager.train_iteration(img, lab))
    tr = GraphedGANTrainer(m, classes)
    tr.capture(img, lab)
    snap = tr.device_snapshot()
    ms, out = _time(lambda: tr.train_iteration(img, lab), steps, warmup)
    tr.device_restore(snap)
    r.update(ms_per_step=round(ms, 4), images_per_s=round(batch * 1000.0 / ms, 1),
             d_loss=float(out[0]), g_loss=float(out[1]), fake_groups=tr._fg)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--dtypes', default='float32,bfloat16')
    ap.add_argument('--data', default='CIFAR10,Omniglot')
    ap.add_argument('--no-mcgan', action='store_true')
    ap.add_argument('--no-launch-count', action='store_true', help='skip torch.profiler (under an external profiler)')
    a = ap.parse_args()
    res = {'workload': 'cgan_train', 'batch': a.batch, 'steps': a.steps, 'config': '5 D + 1 G updates, Adam 2e-4 (0.5, 0.999)',
           'device': torch.cuda.get_device_name(0)}
    for data in a.data.split(','):
        for dt in a.dtypes.split(','):
            res[f'cgan/{data}/{dt}'] = run('cgan', data, dt, a.batch, a.steps, a.warmup, not a.no_launch_count)
            if not a.no_mcgan:
                res[f'mcgan/{data}/{dt}'] = run('mcgan', data, dt, a.batch, a.steps, a.warmup, False)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
