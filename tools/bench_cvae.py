#!/usr/bin/env python3
"""CVAE training step (train_vae.py:98-126) on the HIP path: ms/step of the graph-replayed VAETrainer at B = 128 on the config
widths (hidden [64, 128, 256], latent 128, embedding 32) with 10 modes (CIFAR10, 3x32x32) and 1623 modes (Omniglot, 1x32x32),
fp32 and bf16, with MCVAE's graphed step (10 modes, same dtype) measured in the same run as the yardstick; and the CVAE-only
launches timed on their own at the 10-mode shapes (the encoder input, the first stage's 40-channel im2col next to MCVAE's
8-channel one, the latent pair, the encoder embedding gradient) and the HIP-library calls of one eager step counted.  Prints one JSON line.
usage: tools/bench_cvae.py [--batch 128] [--steps 30] [--warmup 5] [--dtypes float32,bfloat16] [--modes 10,1623] [--no-mcvae]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

DTYPES = {'float32': torch.float32, 'bfloat16': torch.bfloat16}


def _model(name, modes, dtype_name):
    from mcgen_amd import models
    from mcgen_amd.config import cfg
    channels = 1 if modes == 1623 else 3
    cfg.update(model_name=name, data_name='Omniglot' if modes == 1623 else 'CIFAR10', device='cuda', classes_size=modes,
               controller_rate=0.5, data_shape=[channels, 32, 32], compute_dtype=dtype_name)
    cfg['vae'] = {'hidden_size': [64, 128, 256], 'latent_size': 128, 'num_res_block': 2, 'embedding_size': 32}
    torch.manual_seed(0)
    m = getattr(models, name)().cuda()
    return m.set_compute_dtype(DTYPES[dtype_name]), channels


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
    from mcgen_amd.trainer import VAETrainer
    m, channels = _model(name, modes, dtype_name)
    g = torch.Generator(device='cuda').manual_seed(1)
    img = torch.rand(batch, channels, 32, 32, device='cuda', generator=g) * 2 - 1
    lab = torch.randint(0, modes, (batch,), device='cuda', generator=g)
    tr = VAETrainer(m)
    tr.capture(img, lab)
    ms, loss = _time(lambda: tr.train_iteration(img, lab), steps, warmup)
    return {'ms_per_step': round(ms, 4), 'images_per_s': round(batch / ms * 1e3), 'loss': float(loss)}


def library_calls(name, dtype_name, batch):
    """Calls into the HIP library during one eager step (forward, backward, clip, Adam); torch's own tensor ops not counted."""
    from mcgen_amd import ops
    from mcgen_amd.trainer import VAETrainer
    m, channels = _model(name, 10, dtype_name)
    img = torch.rand(batch, channels, 32, 32, device='cuda') * 2 - 1
    lab = torch.randint(0, 10, (batch,), device='cuda')
    tr = VAETrainer(m)
    tr.train_iteration(img, lab)
    seen, orig = [], ops.check
    ops.check = lambda rc, what='': (seen.append(what), orig(rc, what))[1]
    try:
        tr.train_iteration(img, lab)
    finally:
        ops.check = orig
    return len(seen)


def launches(dtype_name, batch, steps, warmup):
    """us per call of the launches CVAE adds to MCVAE's step, eager, at the 10-mode config shapes."""
    from mcgen_amd import ops
    dt = DTYPES[dtype_name]
    g = torch.Generator(device='cuda').manual_seed(2)
    img = torch.rand(batch, 3, 32, 32, device='cuda', generator=g) * 2 - 1
    lab = torch.randint(0, 10, (batch,), device='cuda', generator=g)
    w = torch.randn(32, 10, device='cuda', generator=g)
    x40 = ops.cvae_enc_input(img, w, lab, dt)
    x8 = ops.to_nhwc(img, dt)
    wconv = torch.randn(64, 35, 4, 4, device='cuda', generator=g) * 0.05
    d_h = torch.randn(batch, 16, 16, 64, device='cuda', generator=g).to(dt)
    ml = torch.randn(batch, 256, device='cuda', generator=g).to(dt)
    eps = torch.randn(batch, 128, device='cuda', generator=g)
    mu, logvar, _, _ = ops.cvae_latent_fwd(ml, eps, w, lab, 128)
    dz = torch.randn(batch, 160, device='cuda', generator=g).to(dt)
    dw = torch.empty(32, 10, device='cuda')
    de = torch.randn(batch, 32, device='cuda', generator=g)
    jobs = {'enc_input': lambda: ops.cvae_enc_input(img, w, lab, dt),
            'to_nhwc_8ch(mcvae)': lambda: ops.to_nhwc(img, dt),
            'im2col_40ch': lambda: ops.im2col(x40, 4, 4, 1, 1, stride=2),
            'im2col_8ch(mcvae)': lambda: ops.im2col(x8, 4, 4, 1, 1, stride=2),
            'latent_fwd': lambda: ops.cvae_latent_fwd(ml, eps, w, lab, 128),
            'latent_bwd': lambda: ops.cvae_latent_bwd(dz, mu, logvar, eps, 1.0 / img.numel(), 32),
            'enc_dembed(2 launches)': lambda: ops.cvae_enc_dembed(d_h, wconv, 3, 32),
            'embed_bwd': lambda: ops.cgan_embed_bwd(de, lab, dw)}
    return {k: round(_time(fn, steps, warmup)[0] * 1e3, 2) for k, fn in jobs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--dtypes', default='float32,bfloat16')
    ap.add_argument('--modes', default='10,1623')
    ap.add_argument('--no-mcvae', action='store_true')
    a = ap.parse_args()
    res = {'workload': 'cvae_train', 'batch': a.batch, 'steps': a.steps, 'config': 'hidden [64,128,256], latent 128, embedding 32, '
           '2 residual blocks, 32x32 images (3 channels with 10 modes, 1 with 1623), Adam 3e-4, clip 1',
           'device': torch.cuda.get_device_name(0)}
    for dt in a.dtypes.split(','):
        for modes in map(int, a.modes.split(',')):
            res[f'cvae/{modes}/{dt}'] = train_step('cvae', modes, dt, a.batch, a.steps, a.warmup)
        if not a.no_mcvae:
            res[f'mcvae/10/{dt}'] = train_step('mcvae', 10, dt, a.batch, a.steps, a.warmup)
        res[f'launch_us/{dt}'] = launches(dt, a.batch, a.steps, a.warmup)
    res['library_calls_per_step'] = {n: library_calls(n, 'bfloat16', a.batch) for n in (('cvae',) if a.no_mcvae else ('cvae', 'mcvae'))}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
