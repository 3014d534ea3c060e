#!/usr/bin/env python3
"""CPixelCNN training step (train_pixelcnn.py:108-121) on the HIP path: ms/step of the graph-replayed PixelCNNTrainer at
B = 128 on configs[4] shapes (15 layers, hidden 128, 512 codes, 8x8 code maps) with 10 and 1623 modes, fp32 and bf16,
with MCPixelCNN's graphed step (10 modes, same dtype) measured in the same run as the yardstick; and `sample` of 1000
code maps per dtype (10 modes).  Prints one JSON line.
usage: tools/bench_cpixelcnn.py [--batch 128] [--steps 30] [--warmup 5] [--dtypes float32,bfloat16] [--modes 10,1623]
                                [--samples 1000] [--no-mcpixelcnn]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _model(name, modes, dtype_name):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name=name, device='cuda', classes_size=modes, controller_rate=0.5, compute_dtype=dtype_name)
    cfg['pixelcnn'] = {'num_layer': 15, 'hidden_size': 128, 'num_embedding': 512}
    torch.manual_seed(0)
    m = getattr(models, name)().cuda()
    return m.set_compute_dtype({'float32': torch.float32, 'bfloat16': torch.bfloat16}[dtype_name])


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


def train_step(name, modes, dtype_name, batch, steps, warmup):
    from mcgen_amd.trainer import PixelCNNTrainer
    m = _model(name, modes, dtype_name)
    g = torch.Generator(device='cuda').manual_seed(1)
    codes = torch.randint(0, 512, (batch, 8, 8), device='cuda', generator=g)
    lab = torch.randint(0, modes, (batch,), device='cuda', generator=g)
    tr = PixelCNNTrainer(m)
    tr.capture(codes, lab)
    ms, loss = _time(lambda: tr.train_iteration(codes, lab), steps, warmup)
    return {'ms_per_step': round(ms, 4), 'loss': float(loss)}


def sample(name, dtype_name, n, reps):
    m = _model(name, 10, dtype_name)
    m.train(False)
    lab = torch.arange(n, device='cuda') % 10
    ms, x = _time(lambda: m.sample(lab), reps, 1)
    return {'ms_per_call': round(ms, 3), 'samples': n, 'codes_in_range': bool(int(x.min()) >= 0 and int(x.max()) < 512)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--dtypes', default='float32,bfloat16')
    ap.add_argument('--modes', default='10,1623')
    ap.add_argument('--samples', type=int, default=1000)
    ap.add_argument('--no-mcpixelcnn', action='store_true')
    a = ap.parse_args()
    res = {'workload': 'cpixelcnn_train', 'batch': a.batch, 'steps': a.steps, 'config': 'configs[4]: 15 layers, hidden 128, '
           '512 codes, 8x8 maps, Adam 3e-4, clip 1', 'device': torch.cuda.get_device_name(0)}
    for dt in a.dtypes.split(','):
        for modes in map(int, a.modes.split(',')):
            res[f'cpixelcnn/{modes}/{dt}'] = train_step('cpixelcnn', modes, dt, a.batch, a.steps, a.warmup)
        if not a.no_mcpixelcnn:
            res[f'mcpixelcnn/10/{dt}'] = train_step('mcpixelcnn', 10, dt, a.batch, a.steps, a.warmup)
        if a.samples:
            res[f'cpixelcnn_sample/{dt}'] = sample('cpixelcnn', dt, a.samples, 3)
            if not a.no_mcpixelcnn:
                res[f'mcpixelcnn_sample/{dt}'] = sample('mcpixelcnn', dt, a.samples, 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
