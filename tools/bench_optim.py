#!/usr/bin/env python3
"""The fused optimizer launches (mcgen_sgd, mcgen_rmsprop, mcgen_adamax of csrc/optim_ops.hip) next to mcgen_adam: us per
launch and achieved bytes per second over one flat fp32 buffer of the CIFAR-10 generator's size (4321290) and of a tenth
of it.  The kernels alternate inside every timing window of the same run; the figure of a kernel is the median over the
windows, its spread the range over them.  Bytes are the streams a kernel reads and writes: p (read + write), g (read)
and every state buffer (read + write).  `meets_adam`: the kernel's median bytes/s reaches mcgen_adam's at that size less
the spread of mcgen_adam's windows.  Writes profiles/optim_bench.json (--out) and prints the same JSON on one line.
usage: tools/bench_optim.py [--sizes 4321290,432128] [--windows 11] [--reps 500] [--out profiles/optim_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

LR, WD = 1e-6, 0.0


def _jobs(n):
    """name -> (launch, bytes per element): every kernel on its own buffers."""
    from mcgen_amd import ops
    gen = torch.Generator(device='cuda').manual_seed(n)
    new = lambda scale=1.0: torch.randn(n, device='cuda', generator=gen) * scale       # noqa: E731
    pos = lambda: torch.rand(n, device='cuda', generator=gen) * 1e-4 + 1e-8            # noqa: E731
    step = lambda: torch.zeros(2, dtype=torch.int64, device='cuda')                    # noqa: E731
    g = new()
    b = {k: (new(0.05), new(1e-3), pos(), step()) for k in ('adam', 'sgd', 'sgd_momentum', 'rmsprop', 'rmsprop_momentum', 'adamax')}
    return {
        'adam': (lambda p, a, s, t: ops.adam(p, g, a, s, t, LR, (0.5, 0.999), 1e-8, WD), 28),
        'sgd': (lambda p, a, s, t: ops.sgd(p, g, None, t, LR, 0.0, WD), 12),
        'sgd_momentum': (lambda p, a, s, t: ops.sgd(p, g, a, t, LR, 0.9, WD), 20),
        'rmsprop': (lambda p, a, s, t: ops.rmsprop(p, g, s, None, t, LR, 0.99, 1e-8, 0.0, WD), 20),
        'rmsprop_momentum': (lambda p, a, s, t: ops.rmsprop(p, g, s, a, t, LR, 0.99, 1e-8, 0.9, WD), 28),
        'adamax': (lambda p, a, s, t: ops.adamax(p, g, a, s, t, LR, (0.9, 0.999), 1e-8, WD), 28),
    }, b


def measure(n, windows, reps):
    jobs, bufs = _jobs(n)
    for name, (fn, _) in jobs.items():                       # warm up every kernel at this size
        for _ in range(5):
            fn(*bufs[name])
    torch.cuda.synchronize()
    us = {name: [] for name in jobs}
    for _ in range(windows):
        for name, (fn, _) in jobs.items():                   # the kernels alternate inside every window
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(reps):
                fn(*bufs[name])
            e.record()
            torch.cuda.synchronize()
            us[name].append(s.elapsed_time(e) * 1e3 / reps)
    out = {}
    for name, (_, bpe) in jobs.items():
        gbps = sorted(n * bpe / (t * 1e-6) / 1e9 for t in us[name])
        out[name] = {'bytes_per_element': bpe, 'us_median': round(statistics.median(us[name]), 3),
                     'us_min': round(min(us[name]), 3), 'us_max': round(max(us[name]), 3),
                     'gbytes_per_s_median': round(statistics.median(gbps), 1), 'gbytes_per_s_min': round(gbps[0], 1),
                     'gbytes_per_s_max': round(gbps[-1], 1)}
        assert all(torch.isfinite(t).all() for t in bufs[name][:3]), name
    adam = out['adam']
    floor = adam['gbytes_per_s_median'] - (adam['gbytes_per_s_max'] - adam['gbytes_per_s_min'])
    for name, r in out.items():
        if name != 'adam':
            r['meets_adam'] = r['gbytes_per_s_median'] >= floor
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='4321290,432128')
    ap.add_argument('--windows', type=int, default=11)
    ap.add_argument('--reps', type=int, default=500)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'optim_bench.json'))
    a = ap.parse_args()
    res = {'workload': 'optimizer_launch', 'date': time.strftime('%Y-%m-%d'), 'device': torch.cuda.get_device_name(0),
           'windows': a.windows, 'launches_per_window': a.reps,
           'note': 'eager launches back to back on one stream; the buffers of one kernel (at most 4 x 17 MB) fit the 256 MB '
                   'Infinity Cache, so bytes/s is a cache-assisted rate and comparable between the kernels only'}
    for n in map(int, a.sizes.split(',')):
        res[f'n={n}'] = measure(n, a.windows, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
