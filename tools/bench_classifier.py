#!/usr/bin/env python3
"""Classifier training step (train_classifier.py:104-113) on the HIP path: ms/step of the graph-replayed ClassifierTrainer
at B = 128 for COIL100 ([3,32,32], 100 classes) and Omniglot ([1,32,32], 1623 classes), fp32 and bf16, next to two
yardsticks measured in the same process: the driver's `--engine autograd` loop (the model's autograd bridge +
torch.optim.Adam + clip_grad_norm_) and plain torch-ROCm autograd on the same nn.Module (its Conv2d / BatchNorm2d /
MaxPool2d / Linear children called directly).  Also reports the kernel launches of one eager HIP step (torch.profiler)
and which convolution form / weight-gradient family every launch of the step took.  Prints one JSON line.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel split (profiles/classifier_kernel_stats.csv).
usage: tools/bench_classifier.py [--batch 128] [--steps 50] [--warmup 5] [--dtypes float32,bfloat16] [--data COIL100,Omniglot]
                                 [--no-yardstick] [--no-launch-count]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CLASSES = {'COIL100': ([3, 32, 32], 100), 'Omniglot': ([1, 32, 32], 1623)}
FORMS = ('tiled', 'skinny', 'smap', 'px1', 'c8', 'head')


def _model(data, dtype_name):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    shape, classes = CLASSES[data]
    cfg.update(data_name=data, model_name='classifier', device='cuda', compute_dtype=dtype_name, classes_size=classes,
               data_shape=list(shape))
    cfg['classifier'] = {'hidden_size': [8, 16, 32, 64]}
    torch.manual_seed(0)
    m = models.classifier().cuda()
    m.set_compute_dtype({'float32': torch.float32, 'bfloat16': torch.bfloat16}[dtype_name])
    return m, shape, classes


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
    """GPU kernels of one call of `fn`, counted by torch.profiler (None if the profiler is unavailable)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:                                                          # noqa: BLE001
        return None


def run(data, dtype_name, batch, steps, warmup, yardstick, count=True):
    from mcgen_amd import ops
    from mcgen_amd.trainer import ClassifierTrainer
    m, shape, classes = _model(data, dtype_name)
    g = torch.Generator(device='cuda').manual_seed(1)
    img = torch.rand(batch, *shape, device='cuda', generator=g) * 2 - 1
    lab = torch.randint(0, classes, (batch,), device='cuda', generator=g)
    tr = ClassifierTrainer(m, lr=1e-2)
    # dispatch of one eager step: conv form per launch (forward, head, dgrad) and weight-gradient family per layer
    ops.KERNEL_LOG, ops.WGRAD_LOG = [], []
    tr.train_iteration(img, lab)
    forms, wg = [FORMS[k] for k in ops.KERNEL_LOG], list(ops.WGRAD_LOG)
    ops.KERNEL_LOG = ops.WGRAD_LOG = None
    r = {'conv_forms': forms, 'wgrad_families': wg, 'launches_per_step': _launches(lambda: tr.train_iteration(img, lab)) if count else None}
    tr.capture(img, lab)
    ms, loss = _time(lambda: tr.train_iteration(img, lab), steps, warmup)
    r.update(ms_per_step=round(ms, 4), images_per_s=round(batch * 1000.0 / ms, 1), loss=float(loss))
    if not yardstick:
        return r
    # --engine autograd of the driver: the autograd bridge (HIP kernels) + torch.optim.Adam + clip_grad_norm_
    mb, _, _ = _model(data, dtype_name)
    opt = torch.optim.Adam(mb.parameters(), lr=1e-2)
    mb.train(True)

    def bridge():
        opt.zero_grad()
        out = mb({'img': img, 'label': lab})
        out['loss'].backward()
        torch.nn.utils.clip_grad_norm_(mb.parameters(), 1)
        opt.step()
        return out['loss']
    ms, _ = _time(bridge, max(5, steps // 5), 2)
    r['engine_autograd_ms_per_step'] = round(ms, 4)
    if dtype_name == 'float32':
        # plain torch-ROCm autograd on the same module tree (fp32, MIOpen convolutions)
        mt, _, _ = _model(data, dtype_name)
        opt2 = torch.optim.Adam(mt.parameters(), lr=1e-2)
        mt.train(True)

        def eager():
            opt2.zero_grad()
            loss = F.cross_entropy(mt.classifier(mt.blocks(img).flatten(1)), lab)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(mt.parameters(), 1)
            opt2.step()
            return loss
        ms, _ = _time(eager, max(5, steps // 5), 3)
        r['torch_autograd_ms_per_step'] = round(ms, 4)
        r['torch_autograd_launches_per_step'] = _launches(eager) if count else None
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--dtypes', default='float32,bfloat16')
    ap.add_argument('--data', default='COIL100,Omniglot')
    ap.add_argument('--no-yardstick', action='store_true')
    ap.add_argument('--no-launch-count', action='store_true', help='skip torch.profiler (under an external profiler)')
    a = ap.parse_args()
    res = {'workload': 'classifier_train', 'batch': a.batch, 'steps': a.steps, 'config': 'hidden [8, 16, 32, 64], Adam 1e-2',
           'device': torch.cuda.get_device_name(0)}
    for data in a.data.split(','):
        for dt in a.dtypes.split(','):
            res[f'{data}/{dt}'] = run(data, dt, a.batch, a.steps, a.warmup, not a.no_yardstick, not a.no_launch_count)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
