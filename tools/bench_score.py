#!/usr/bin/env python3
"""InceptionScore + FID of a generated set as compat/train_gan.py asks for them after every epoch, at the two real shapes --
COIL100 (10 000 generated images, 100 classes) and Omniglot (32 460 generated images, 1623 classes), 1024 features in both --
through `mcgen_amd.metrics.GanScorer` (one classifier pass, streaming float64 accumulators in csrc/score_ops.hip) against the
path it stands beside, `metrics.inception_score` + `metrics.fid` on the same images (two classifier passes, concatenated
float64 matrices, generic torch reductions).  The classifier has random weights; the images are pre-generated uniform noise in
chunks of 500, as the driver's test() produces them.  Everything is timed host to host (perf_counter around calls that end
synchronised), after warm-up calls, as the median over windows of `--calls` calls each.  One `score` is also split into its
three parts, each timed on its own: the classifier, the two accumulate calls per chunk, the finalisation (moments, the
`eigvalsh` behind tr sqrt(S1 S2), the one transfer).  Last, the float64 rank-n update alone on the whole [n, 1024] feature
matrix against the library GEMM `x.double().T @ x.double()` (the widening copy included: the kernel needs none), with the
fraction of the float64 matrix peak the kernel reaches.  Writes one JSON document.
usage: tools/bench_score.py [--windows 5] [--calls 3] [--warmup 2] [--out profiles/score_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CASES = [('COIL100', 10000, 4096), ('Omniglot', 32460, 4096)]          # data, generated images, real images
F64_MATRIX_PEAK = 78.6e12                                              # MI355X data sheet: FP64 matrix, FLOP/s


def _median_ms(fn, windows, calls, warmup):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            out = fn()
        torch.cuda.synchronize()
        per_call.append((time.perf_counter() - t0) / calls * 1e3)
    return statistics.median(per_call), out


def _checkpoint(data_name, directory):
    """models.classifier() for `data_name` with its random initial weights, in the reference's checkpoint layout."""
    from mcgen_amd import models
    from mcgen_amd.checkpoint import save
    from mcgen_amd.config import cfg, process_control
    cfg.update(data_name=data_name, model_name='classifier', device='cuda', subset='label')
    cfg.pop('classes_size', None)
    process_control()
    torch.manual_seed(0)
    m = models.classifier()
    path = os.path.join(directory, f'0_{data_name}_label_classifier_best.pt')
    save({'epoch': 1, 'model_dict': {k: v.cpu() for k, v in m.state_dict().items()}}, path)
    return path, list(cfg['data_shape'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score_bench.json'))
    a = ap.parse_args()
    from mcgen_amd import metrics, ops
    timed = lambda fn: _median_ms(fn, a.windows, a.calls, a.warmup)      # noqa: E731
    res = {'workload': 'InceptionScore + FID per epoch (GanScorer)', 'device': torch.cuda.get_device_name(0),
           'method': f'host to host, median of {a.windows} windows x {a.calls} calls, {a.warmup} warm-up calls',
           'f64_matrix_peak_flops': F64_MATRIX_PEAK, 'cases': []}
    with tempfile.TemporaryDirectory() as tmp:
        for i, (name, n, n_real) in enumerate(CASES):
            path, shape = _checkpoint(name, tmp)
            g = torch.Generator(device='cuda').manual_seed(100 + i)
            img = torch.rand(n, *shape, device='cuda', generator=g) * 2 - 1
            real = torch.rand(n_real, *shape, device='cuda', generator=g) * 2 - 1
            chunks = img.split(500)
            scorer = metrics.GanScorer(name, real, checkpoint=path)
            model, acc = scorer.model, scorer.acc
            total_ms, got = timed(lambda: scorer.score(chunks))

            def classify():
                with torch.no_grad():
                    return [model.score_outputs({'img': x}) for c in chunks for x in c.split(scorer.batch_size)]
            classifier_ms, outs = timed(classify)

            def accumulate():
                acc.reset()
                for logits, feature in outs:
                    acc.add(logits, feature)
            accumulate_ms, _ = timed(accumulate)
            mu1, s1, r1 = scorer._real

            def finalise():
                _, mu2, s2 = acc.moments()
                return torch.stack([acc.inception_score_tensor(), metrics._fid_tensor(mu1, s1, mu2, s2, r1)]).tolist()
            accumulate()
            finalise_ms, _ = timed(finalise)

            def parent():
                return (metrics.inception_score(img, name, model=model), metrics.fid(img, name, real=real, model=model))
            parent_ms, want = timed(parent)
            # the rank-n update alone, on all n rows at once
            feature = torch.cat([f for _, f in outs])
            d = feature.shape[1]
            fsum, gram = torch.zeros(d, dtype=torch.float64, device='cuda'), torch.zeros(d, d, dtype=torch.float64, device='cuda')
            work = torch.empty(ops.score_moments_work(n, d), dtype=torch.float64, device='cuda')
            moments_ms, _ = timed(lambda: ops.score_moments(feature, work, fsum, gram))
            gemm_ms, ref = timed(lambda: feature.double().t() @ feature.double())
            gram.zero_(), fsum.zero_()
            ops.score_moments(feature, work, fsum, gram)
            tiles = -(-d // 64)
            executed = 2.0 * n * 32 * 32 * (4 * tiles * (tiles - 1) // 2 + 3 * tiles)      # quadrants of the upper triangle
            case = {'data': name, 'generated': n, 'real': n_real, 'classes': acc.classes, 'features': d,
                    'score_ms': round(total_ms, 3), 'classifier_ms': round(classifier_ms, 3), 'accumulate_ms': round(accumulate_ms, 3),
                    'finalise_ms': round(finalise_ms, 3), 'concatenating_ms': round(parent_ms, 3),
                    'speedup': round(parent_ms / total_ms, 2),
                    'inception_score': got['InceptionScore'], 'inception_score_concatenating': want[0],
                    'inception_score_difference': abs(got['InceptionScore'] - want[0]),
                    'fid': got['FID'], 'fid_concatenating': want[1], 'fid_difference': abs(got['FID'] - want[1]),
                    'moments_all_rows_ms': round(moments_ms, 3), 'library_gemm_f64_ms': round(gemm_ms, 3),
                    'rank_n_update_flop': 2.0 * n * d * d, 'executed_flop': executed,
                    'fraction_of_f64_matrix_peak': round(executed / (moments_ms * 1e-3) / F64_MATRIX_PEAK, 4),
                    'gram_max_difference_to_gemm': float((gram - ref).abs().max()), 'gram_symmetric': bool(torch.equal(gram, gram.t()))}
            res['cases'].append(case)
            print(json.dumps(case), flush=True)
            del img, real, outs, feature, scorer
            torch.cuda.empty_cache()
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
