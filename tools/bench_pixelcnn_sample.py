#!/usr/bin/env python3
"""MCPixelCNN ancestral sampling at N samples on the configs[4] model (hidden 128, 15 layers, 512 codes, 10 classes):
`MCGatedPixelCNN.sample` (csrc/pixelcnn_sample.hip: 8 row launches + 64 column launches, every pixel of every layer
computed once) against `generate` (64 full eval forwards, the reference's loop), fp32 and bf16.  Prints one JSON line
(ms per call of N samples, the speed-up, and how many of the draws agree when both decode greedily).  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel split (profiles/pixelcnn_sample_kernel_stats.csv).
usage: tools/bench_pixelcnn_sample.py [--n 1000] [--steps 5] [--warmup 1] [--generate-steps 2] [--dtypes float32,bfloat16]
                                      [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DTYPES = {'float32': torch.float32, 'bfloat16': torch.bfloat16}


def _model(dtype):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name='mcpixelcnn', device='cuda', classes_size=10, controller_rate=0.5, compute_dtype='float32')
    cfg['pixelcnn'] = {'num_layer': 15, 'hidden_size': 128, 'num_embedding': 512}
    torch.manual_seed(0)
    return models.mcpixelcnn().cuda().train(False).set_compute_dtype(dtype)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--generate-steps', type=int, default=2)
    ap.add_argument('--dtypes', default='float32,bfloat16')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'workload': 'mcpixelcnn_sample', 'n': a.n, 'map': [8, 8],
           'config': 'hidden 128, 15 layers, 512 codes, 10 classes', 'device': torch.cuda.get_device_name(0)}
    lab = (torch.arange(a.n, device='cuda') % 10)
    for name in a.dtypes.split(','):
        m = _model(DTYPES[name])
        with torch.no_grad():
            t_s, _ = _time(lambda: m.sample(lab), a.steps, a.warmup)
            t_g, _ = _time(lambda: m.generate(lab), a.generate_steps, 1)
            greedy = m.sample(lab, greedy=True)
            slow = m.generate(lab, sampler=lambda p: p.argmax(-1))
        res[name] = {'sample_ms': round(t_s, 3), 'generate_ms': round(t_g, 3), 'speedup': round(t_g / t_s, 2),
                     'samples_per_s': round(a.n / t_s * 1e3, 1),
                     'greedy_agreement': round(float((greedy == slow).float().mean()), 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
