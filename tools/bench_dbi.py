#!/usr/bin/env python3
"""Davies-Bouldin index of a created set at the three real shapes -- 10 000 x 3072 in 10 clusters (CIFAR10), 10 000 x 3072 in
100 clusters (COIL100), 32 460 x 1024 in 1623 clusters (Omniglot) -- on device tensors: `mcgen_amd.metrics.davies_bouldin`
(csrc/dbi_ops.hip, one float leaves HBM) against the path it replaces, a device-to-host copy followed by scikit-learn's
davies_bouldin_score.  Both are timed host to host (perf_counter around a call that ends synchronised), after warm-up calls,
as the median over windows of `--calls` calls each.  Writes one JSON document with both times, both values and their relative
difference per shape.
usage: tools/bench_dbi.py [--windows 5] [--calls 3] [--host-windows 3] [--warmup 2] [--out profiles/dbi_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [('CIFAR10', 10000, 3072, 10), ('COIL100', 10000, 3072, 100), ('Omniglot', 32460, 1024, 1623)]


def _case(n, d, k, seed):
    """tanh(centre[label] + 0.5 noise), centres ~ 0.3 N(0, 1): the inputs of tests/dbi_ref.py at the real shapes."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    label = (torch.arange(n, device='cuda') % k)[torch.randperm(n, device='cuda', generator=g)]
    centre = 0.3 * torch.randn(k, d, device='cuda', generator=g)
    return torch.tanh(centre[label] + 0.5 * torch.randn(n, d, device='cuda', generator=g)), label


def _median_ms(fn, windows, calls, warmup):
    for _ in range(warmup):
        out = fn()
    per_call = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            out = fn()
        torch.cuda.synchronize()
        per_call.append((time.perf_counter() - t0) / calls * 1e3)
    return statistics.median(per_call), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--host-windows', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dbi_bench.json'))
    a = ap.parse_args()
    from sklearn.metrics import davies_bouldin_score
    from mcgen_amd.metrics import davies_bouldin
    res = {'workload': 'davies_bouldin', 'device': torch.cuda.get_device_name(0),
           'method': f'median of {a.windows} windows x {a.calls} calls (device), {a.host_windows} windows x 1 call (host), '
                     f'{a.warmup} / 1 warm-up calls', 'shapes': []}
    for i, (name, n, d, k) in enumerate(SHAPES):
        x, label = _case(n, d, k, 100 + i)
        dev_ms, dev = _median_ms(lambda: davies_bouldin(x, label), a.windows, a.calls, a.warmup)
        host_ms, host = _median_ms(lambda: float(davies_bouldin_score(x.cpu().numpy(), label.cpu().numpy())), a.host_windows, 1, 1)
        res['shapes'].append({'data': name, 'rows': n, 'columns': d, 'clusters': k, 'device_ms': round(dev_ms, 3),
                              'host_sklearn_ms': round(host_ms, 3), 'speedup': round(host_ms / dev_ms, 2),
                              'device_value': dev, 'sklearn_float32_value': host, 'relative_difference': abs(dev - host) / host})
        print(json.dumps(res['shapes'][-1]), flush=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
