#!/usr/bin/env python3
"""VQ-VAE training step (train_vqvae.py:99-112) on the HIP path: ms/step and images/s of the graph-replayed
VQVAETrainer at the shipped config (hidden [128, 128], D 64, K 512, CIFAR-10 32x32), B = 128, fp32 and bf16; prints one
JSON line.  Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel split (profiles/vqvae_kernel_stats.csv);
`--counts` adds the per-code pixel histogram of the timed batch (max / median pixels per used code).
usage: tools/bench_vqvae.py [--batch 128] [--steps 50] [--warmup 5] [--dtypes float32,bfloat16] [--counts]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def run(dtype_name, batch, steps, warmup, counts):
    from mcgen_amd import models
    from mcgen_amd.config import cfg, process_control
    from mcgen_amd.trainer import VQVAETrainer
    cfg.update(data_name='CIFAR10', model_name='vqvae', ae_name='vqvae', device='cuda', compute_dtype=dtype_name)
    process_control()
    torch.manual_seed(0)
    m = models.vqvae().cuda()
    m.set_compute_dtype({'float32': torch.float32, 'bfloat16': torch.bfloat16}[dtype_name])
    g = torch.Generator(device='cuda').manual_seed(1)
    img = torch.rand(batch, 3, 32, 32, device='cuda', generator=g) * 2 - 1
    tr = VQVAETrainer(m)
    tr.capture(img)
    for _ in range(warmup):
        tr.train_iteration(img)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        loss = tr.train_iteration(img)
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / steps
    r = {'ms_per_step': round(ms, 4), 'images_per_s': round(batch * 1000.0 / ms, 1), 'loss': float(loss)}
    if counts:
        with torch.no_grad():
            out = m._engine().forward(img, False)
        h = torch.bincount(out['code'].flatten(), minlength=m.quantizer.num_embedding)
        used = h[h > 0]
        r['codes_used'] = int(used.numel())
        r['pixels_per_code_max'] = int(used.max())
        r['pixels_per_code_median'] = float(used.float().median())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--dtypes', default='float32,bfloat16')
    ap.add_argument('--counts', action='store_true')
    a = ap.parse_args()
    res = {'workload': 'vqvae_cifar10_train', 'batch': a.batch, 'steps': a.steps, 'config': 'hidden [128, 128], D 64, K 512',
           'device': torch.cuda.get_device_name(0)}
    for dt in a.dtypes.split(','):
        res[dt] = run(dt, a.batch, a.steps, a.warmup, a.counts)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
