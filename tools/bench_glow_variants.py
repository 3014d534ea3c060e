#!/usr/bin/env python3
"""MCGlow training step (train_glow.py:108-121) on the HIP path for the four combinations of coupling form (glow.affine) and
1x1 convolution (glow.conv_lu): ms/step of the graph-replayed GlowTrainer at configs[3] shapes (Omniglot 1x32x32, 1623 modes,
hidden 512, K = 16, L = 3, B = 128), bf16 and fp32.  The four trainers live in one process and their timed windows alternate
(window i of every combination before window i + 1 of any), so drift of the device hits all of them alike.  Next to it: the
batched float64 factorisation launch of the plain form alone (48 matrices: 16 each of C = 4/8/16, and of 12/24/48) beside
mcgen_invconv_weight_batch on LU modules of the same sizes, and the HIP-library calls of one eager step per combination.
Prints one JSON line and writes it to --out.  No pass/fail threshold: a record.
usage: tools/bench_glow_variants.py [--batch 128] [--steps 20] [--warmup 3] [--trials 5] [--dtypes bfloat16,float32]
                                    [--out profiles/glow_variants_bench.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DTYPES = {'float32': torch.float32, 'bfloat16': torch.bfloat16}
COMBOS = [(True, True), (False, True), (True, False), (False, False)]           # (affine, conv_lu); the first is the table's
CHANNELS, MODES = 1, 1623


def _name(affine, conv_lu):
    return ('affine' if affine else 'additive') + '+' + ('lu' if conv_lu else 'plain')


def _model(affine, conv_lu, dtype_name):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    cfg.update(model_name='mcglow', data_name='Omniglot', device='cuda', classes_size=MODES, controller_rate=0.5,
               data_shape=[CHANNELS, 32, 32], compute_dtype=dtype_name)
    cfg['glow'] = {'hidden_size': 512, 'K': 16, 'L': 3, 'affine': affine, 'conv_lu': conv_lu}
    torch.manual_seed(0); np.random.seed(0)
    return models.mcglow().cuda().set_compute_dtype(DTYPES[dtype_name])


def _inputs(m, batch):
    g = torch.Generator(device='cuda').manual_seed(1)
    img = torch.rand(batch, CHANNELS, 32, 32, device='cuda', generator=g) * 2 - 1
    lab = torch.randint(0, MODES, (batch,), device='cuda', generator=g)
    m.train(True)
    with torch.no_grad():                                 # the data-dependent ActNorm initialisation (train_glow.py:60-67)
        m({'img': img, 'label': lab})
    return img, lab


def _window(fn, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps, out


def _stats(ms, digits=4, scale=1.0):
    ms = sorted(m * scale for m in ms)
    return {'median': round(ms[len(ms) // 2], digits), 'min': round(ms[0], digits), 'max': round(ms[-1], digits)}


def train_steps(dtype_name, batch, steps, warmup, trials):
    from mcgen_amd import ops
    from mcgen_amd.trainer import GlowTrainer
    runs = {}
    for affine, conv_lu in COMBOS:
        m = _model(affine, conv_lu, dtype_name)
        img, lab = _inputs(m, batch)
        tr = GlowTrainer(m)
        seen, orig = [], ops.check                        # the library calls of one eager step, before the capture
        tr.train_iteration(img, lab)
        ops.check = lambda rc, what='': (seen.append(what), orig(rc, what))[1]
        try:
            tr.train_iteration(img, lab)
        finally:
            ops.check = orig
        tr.capture(img, lab)
        fn = (lambda tr=tr, img=img, lab=lab: tr.train_iteration(img, lab))
        for _ in range(warmup):
            fn()
        runs[_name(affine, conv_lu)] = dict(fn=fn, ms=[], calls=len(seen))
    torch.cuda.synchronize()
    for _ in range(trials):                               # alternated: one window of each combination per round
        for r in runs.values():
            ms, r['loss'] = _window(r['fn'], steps)
            r['ms'].append(ms)
    out = {}
    for k, r in runs.items():
        st = _stats(r['ms'])
        out[k] = {'ms_per_step': st, 'images_per_s': round(batch / st['median'] * 1e3), 'loss': float(r['loss']),
                  'library_calls_per_eager_step': r['calls']}
    return out


def factorisation(sizes, steps, warmup, trials):
    """us per call of the batched launches over 48 matrices, 16 of each size: the plain form's float64 factorisation
    (log|det| and inverse) and the LU form's weight build (no inverse: the training pass takes none)."""
    from mcgen_amd import ops
    from mcgen_amd.models.mcglow import InvConv2d, InvConv2dLU
    torch.manual_seed(0); np.random.seed(0)
    plain = [InvConv2d(c).cuda().weight.detach() for c in sizes for _ in range(16)]
    lus = [InvConv2dLU(c).cuda() for c in sizes for _ in range(16)]
    jobs = {'invconv_plain_batch': lambda: ops.invconv_plain_batch(plain), 'invconv_weight_batch': lambda: ops.invconv_weight_batch(lus)}
    out = {}
    for k, fn in jobs.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        out[k] = _stats([_window(fn, steps)[0] for _ in range(trials)], 2, 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--trials', type=int, default=5, help='timed windows of --steps replays each; median, min and max are reported')
    ap.add_argument('--dtypes', default='bfloat16,float32')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'glow_variants_bench.json'))
    a = ap.parse_args()
    res = {'workload': 'mcglow_variants_train', 'batch': a.batch, 'steps': a.steps, 'warmup': a.warmup, 'trials': a.trials,
           'config': 'Omniglot 1x32x32, 1623 modes, hidden 512, K 16, L 3, Adam 3e-4, clip 1, graph-replayed step; the four '
                     'combinations in one process, windows alternated; per combination `trials` windows of `steps` replays '
                     'between device events: median, min, max',
           'device': torch.cuda.get_device_name(0)}
    for dt in a.dtypes.split(','):
        for k, v in train_steps(dt, a.batch, a.steps, a.warmup, a.trials).items():
            res[f'{k}/{dt}'] = v
    for tag, sizes in (('4/8/16', (4, 8, 16)), ('12/24/48', (12, 24, 48))):
        res[f'launch_us/48 jobs, C = {tag}'] = factorisation(sizes, 200, 20, a.trials)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
