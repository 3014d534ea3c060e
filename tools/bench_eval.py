#!/usr/bin/env python3
"""One evaluation pass of the compat/test_*.py drivers over a fixed synthetic set, per model: the reference's loop (--metrics
host: `Metric.evaluate` and `Logger.append` per batch, every metric ending in a host synchronisation) against the device
evaluator (--metrics device: mcgen_amd.evaluate.DeviceEvaluator, one device-to-host copy per pass).  Both run the same
`EvalDriver.test` in this process on the same randomly initialised model (the time does not depend on the weights) and the same
loader; a pass is timed host to host (perf_counter around passes that end synchronised), after warm-up passes, in windows of
`--passes` passes each, the two modes alternating window by window.  Writes one JSON document with the median, minimum and
maximum over the windows for both modes, the ratio of the medians and both results per model.  (The device mode lays the
loader's NHWC-strided images out before the model, the host mode leaves that to the model: the same copy, in another place.)
usage: tools/bench_eval.py [--images 1024] [--batch 128] [--windows 9] [--passes 10] [--warmup 2] [--models cvae,vqvae,...]
                           [--out profiles/eval_bench.json]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'compat')]

import torch  # noqa: E402

# model -> (dataset, control, test driver module, driver class)
CASES = {'cvae': ('CIFAR10', None, 'test_vae', 'VAETest'), 'vqvae': ('CIFAR10', None, 'test_vqvae', 'VQVAETest'),
         'mcpixelcnn': ('CIFAR10', '0.5', 'test_pixelcnn', 'PixelCNNTest'),
         'classifier': ('COIL100', None, 'test_classifier', 'ClassifierTest'), 'cglow': ('MNIST', None, 'test_glow', 'GlowTest')}


def _setup(name, images, batch):
    """-> (driver, loader, model, ae): what EvalDriver.run_experiment hands to `test`, without checkpoints."""
    import importlib
    import models
    from _single import cfg
    from mcgen_amd.config import process_control
    from mcgen_amd.data import DeviceLoader, synthetic_uint8_dataset
    data, control, module, cls = CASES[name]
    cfg.update(data_name=data, model_name=name, device='cuda:0', subset='label', ae_name='vqvae',
               control={'controller_rate': control} if control else {}, model_tag=f'bench_{name}')
    cfg.pop('classes_size', None)
    process_control()
    torch.manual_seed(0)
    img, label = synthetic_uint8_dataset(images, cfg['data_shape'], cfg['classes_size'], seed=0, device='cuda:0')
    loader = DeviceLoader(img, label, batch, shuffle=True)
    ae = None
    if 'pixelcnn' in name:
        ae = models.vqvae().to('cuda:0')
        ae.train(False)
    model = getattr(models, name)().to('cuda:0')
    if 'glow' in name:                                    # data-dependent ActNorm initialisation (train_glow.py:60-67)
        with torch.no_grad():
            model.train(True)
            model(next(iter(loader)))
    driver = getattr(importlib.import_module(module), cls)()
    driver.grids = False                                  # the grids are file output, the same in both modes
    return driver, loader, model, ae


def _windows_ms(fns, windows, passes, warmup):
    """ms per pass of every mode in `fns`, one list of `windows` values each: the modes take turns window by window, so a drift
    of the clocks or of the box falls on all of them alike."""
    outs = {}
    for name, fn in fns.items():
        for _ in range(warmup):
            outs[name] = fn()
    per_pass = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(passes):
                outs[name] = fn()
            torch.cuda.synchronize()
            per_pass[name].append((time.perf_counter() - t0) / passes * 1e3)
    return per_pass, outs


def _stats(values):
    return {'median_ms': round(statistics.median(values), 3), 'min_ms': round(min(values), 3), 'max_ms': round(max(values), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=1024)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--passes', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--models', default=','.join(CASES))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_bench.json'))
    a = ap.parse_args()
    from logger import Logger
    res = {'workload': 'evaluation pass (compat/test_*.py, EvalDriver.test)', 'device': torch.cuda.get_device_name(0),
           'images': a.images, 'batch': a.batch,
           'method': f'host to host; {a.windows} windows x {a.passes} passes per mode, the two modes alternating window by window, '
                     f'{a.warmup} warm-up passes per mode; median, minimum and maximum over the windows',
           'models': []}
    for name in a.models.split(','):
        driver, loader, model, ae = _setup(name, a.images, a.batch)

        def one_pass(mode):
            driver.mode = mode
            logger = Logger('unused')
            with contextlib.redirect_stdout(io.StringIO()):
                driver.test(loader, model, ae, logger, 1)
            return {k.split('/', 1)[1]: v for k, v in logger.mean.items()}
        per_pass, outs = _windows_ms({'host': lambda: one_pass('host'), 'device': lambda: one_pass('device')}, a.windows, a.passes,
                                     a.warmup)
        host, dev = _stats(per_pass['host']), _stats(per_pass['device'])
        res['models'].append({'model': name, 'data': CASES[name][0], 'metrics': driver.metric_names, 'batches': len(loader),
                              'host': host, 'device': dev, 'host_over_device': round(host['median_ms'] / dev['median_ms'], 3),
                              'host_result': outs['host'], 'device_result': outs['device']})
        print(json.dumps(res['models'][-1]), flush=True)
        del driver, loader, model, ae
        torch.cuda.empty_cache()
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
