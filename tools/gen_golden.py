#!/usr/bin/env python3
"""Generate the committed golden fixtures under tests/golden/ by RUNNING THE
REFERENCE (its ``models``/``modules`` packages, imported on CPU).

Runs only in the build container, where /root/reference exists; the reference
never travels to the GPU box -- only the .npz vectors do.  The reference's
``utils.py``/``data.py`` need torchvision and do not import here, so the cfg
keys that ``process_control`` would derive (utils.py:104-192) are set by hand
and the train loop body (train_gan.py:139-176) is driven around the imported
model with explicitly injected latents.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py [--only NAME]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('MC_REFERENCE', '/root/reference/src')
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, 'tests'))
os.chdir(REF)                     # config.py opens config.yml relatively (config.py:4)
sys.path.insert(0, REF)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from config import cfg  # noqa: E402

import golden_util as gu  # noqa: E402

torch.set_num_threads(8)
OUT = gu.GOLDEN_DIR


def set_gan_cfg(g_hidden, d_hidden, classes, data_name='CIFAR10'):
    cfg['model_name'] = 'mcgan'
    cfg['data_name'] = data_name
    cfg['device'] = 'cpu'
    cfg['classes_size'] = classes
    cfg['controller_rate'] = 0.5
    cfg['data_shape'] = [3, 32, 32]
    cfg['gan'] = {'latent_size': 128, 'generator_hidden_size': list(g_hidden),
                  'discriminator_hidden_size': list(d_hidden), 'embedding_size': 32}


def np_state(sd, prefix='sd/'):
    return {prefix + k: v.detach().cpu().numpy().copy() for k, v in sd.items()}


def save(name, **arrays):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrays)
    print(f'wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB)')


# --------------------------------------------------------------------------- #
def fx_mc_unit():
    """MultimodalController forward/backward, 4-D and 2-D inputs (modules.py:71-76)."""
    from modules import MultimodalController
    torch.manual_seed(0)
    mc = MultimodalController(32, 10, 0.5)
    x4 = torch.randn(4, 32, 4, 4, requires_grad=True)
    x2 = torch.randn(4, 32, requires_grad=True)
    lab = torch.tensor([3, 0, 9, 3])
    ind = F.one_hot(lab, 10).float()
    g4, g2 = torch.randn(4, 32, 4, 4), torch.randn(4, 32)
    o4 = mc([x4, ind])[0]; o4.backward(g4)
    o2 = mc([x2, ind])[0]; o2.backward(g2)
    soft = torch.softmax(torch.randn(4, 10), -1)         # non one-hot indicator
    os_ = mc([x4.detach(), soft])[0]
    ones = MultimodalController(32, 10, 1)                # rate 1 -> identity
    save('mc_unit.npz', codebook=mc.codebook.numpy(), x4=x4.detach().numpy(), x2=x2.detach().numpy(),
         label=lab.numpy(), g4=g4.numpy(), g2=g2.numpy(), out4=o4.detach().numpy(), out2=o2.detach().numpy(),
         dx4=x4.grad.numpy(), dx2=x2.grad.numpy(), soft=soft.numpy(), out_soft=os_.numpy(),
         ones_codebook=ones.codebook.numpy())


def fx_blocks():
    """Single residual blocks of the reference: outputs, input/param grads,
    BN running stats and SN u/v after one and two training forwards."""
    import importlib
    import models  # noqa: F401
    M = sys.modules.get('models.mcgan') or importlib.import_module('models.mcgan')
    from models.utils import make_SpectralNormalization
    set_gan_cfg([16] * 4, [16] * 4, 10)
    torch.manual_seed(3)
    lab = torch.tensor([1, 7, 7, 0, 4, 9])
    ind = F.one_hot(lab, 10).float()
    arrays = {'label': lab.numpy()}

    def run(tag, blk, x):
        for p in blk.parameters():
            torch.nn.init.normal_(p, 0.0, 0.2) if p.dim() > 1 else torch.nn.init.uniform_(p, 0.5, 1.5)
        blk.train(True)
        arrays.update(np_state(blk.state_dict(), f'{tag}/sd0/'))
        x = x.clone().requires_grad_(True)
        out = blk([x, ind])[0]
        g = torch.randn_like(out)
        out.backward(g)
        arrays[f'{tag}/x'] = x.detach().numpy(); arrays[f'{tag}/g'] = g.numpy()
        arrays[f'{tag}/out'] = out.detach().numpy(); arrays[f'{tag}/dx'] = x.grad.numpy()
        for n, p in blk.named_parameters():
            arrays[f'{tag}/grad/{n}'] = p.grad.numpy().copy()
        arrays.update(np_state(blk.state_dict(), f'{tag}/sd1/'))
        out2 = blk([x.detach(), ind])[0]                   # second forward: SN/BN state advances again
        arrays[f'{tag}/out_second'] = out2.detach().numpy()
        arrays.update(np_state(blk.state_dict(), f'{tag}/sd2/'))
        blk.train(False)
        arrays[f'{tag}/out_eval'] = blk([x.detach(), ind])[0].detach().numpy()

    run('gen', M.GenResBlock(16, 16, 10, 0.5, 2), torch.randn(6, 16, 4, 4))
    run('dis_first', M.FirstDisResBlock(3, 16, 10, 0.5).apply(make_SpectralNormalization), torch.randn(6, 3, 8, 8))
    run('dis_s2', M.DisResBlock(16, 16, 10, 0.5, 2).apply(make_SpectralNormalization), torch.randn(6, 16, 8, 8))
    run('dis_s1', M.DisResBlock(16, 16, 10, 0.5, 1).apply(make_SpectralNormalization), torch.randn(6, 16, 4, 4))
    save('mcgan_blocks.npz', **arrays)


def ref_train_iteration(model, opt, img, label, zs, d_iters=5, g_iters=1):
    """train_gan.py:139-176 around the imported model, latents injected."""
    zi = iter(zs)
    for _ in range(d_iters):
        opt['discriminator'].zero_grad(); opt['generator'].zero_grad()
        d_x = model.discriminate(img, label)
        generated = model.generate(label, next(zi))
        d_gz = model.discriminate(generated.detach(), label)
        d_loss = F.relu(1.0 - d_x).mean() + F.relu(1.0 + d_gz).mean()
        d_loss.backward()
        opt['discriminator'].step()
    for _ in range(g_iters):
        opt['discriminator'].zero_grad(); opt['generator'].zero_grad()
        generated = model.generate(label, next(zi))
        g_loss = -model.discriminate(generated, label).mean()
        g_loss.backward()
        opt['generator'].step()
    return d_loss.item(), g_loss.item()


def make_opt(model):
    return {'generator': torch.optim.Adam(model.generator.parameters(), lr=2e-4, betas=(0.5, 0.999)),
            'discriminator': torch.optim.Adam(model.discriminator.parameters(), lr=2e-4, betas=(0.5, 0.999))}


def fx_mcgan_small():
    """Reduced-width MCGAN, reference init (seed 0), 3 train iterations, B=8."""
    import models
    set_gan_cfg([32] * 4, [16] * 4, 10)
    torch.manual_seed(0)
    model = models.mcgan()
    model.train(True)
    arrays = np_state(model.state_dict(), 'sd/')
    B, iters = 8, 3
    img, lab = gu.synthetic_batch(B, 10, seed=1)
    zs = gu.latent_batches(6 * iters + 1, B, 128, seed=2)
    arrays['img'] = img.numpy(); arrays['label'] = lab.numpy()
    arrays['z'] = torch.stack(zs).numpy()
    # single forward/backward probes before any update
    probe = model.generate(lab, zs[-1])
    d_probe = model.discriminate(img, lab)
    arrays['probe_generated'] = probe.detach().numpy()
    arrays['probe_d_real'] = d_probe.detach().numpy()
    arrays.update(np_state(model.state_dict(), 'sd_after_probe/'))
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in arrays.items() if k.startswith('sd/')})
    opt = make_opt(model)
    losses = []
    for it in range(iters):
        losses.append(ref_train_iteration(model, opt, img, lab, zs[6 * it:6 * it + 6]))
    arrays['losses'] = np.array(losses, dtype=np.float64)
    arrays.update(np_state(model.state_dict(), 'sd_final/'))
    model.train(False)
    with torch.no_grad():
        arrays['final_generated_eval'] = model.generate(lab, zs[-1]).numpy()
        arrays['final_d_eval'] = model.discriminate(img, lab).numpy()
    save('mcgan_small.npz', **arrays)


def fx_mcgan_full():
    """Full-size MCGAN (utils.py:156-162) with procedural weights: only inputs
    that cannot be regenerated, losses and digests are stored."""
    import models
    g_hidden, d_hidden = [256] * 4, [128] * 4
    set_gan_cfg(g_hidden, d_hidden, 10)
    torch.manual_seed(0)
    model = models.mcgan()
    shapes = gu.mcgan_shapes(g_hidden, d_hidden, 10)
    ref_shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert shapes == ref_shapes, set(shapes.items()) ^ set(ref_shapes.items())
    sd = gu.procedural_state(shapes, seed=1234, num_mode=10)
    model.load_state_dict(sd)
    model.train(True)
    B = 16
    img, lab = gu.synthetic_batch(B, 10, seed=1)
    zs = gu.latent_batches(6 * 2, B, 128, seed=2)
    arrays = {}
    gen0 = model.generate(lab, zs[0])
    d0 = model.discriminate(img, lab)
    arrays['probe_generated'] = gen0.detach().numpy()[:, :, ::4, ::4].copy()   # strided sample
    arrays['probe_generated_digest'] = gu.checksum(gen0)
    arrays['probe_d_real'] = d0.detach().numpy()
    model.load_state_dict(sd)
    opt = make_opt(model)
    losses = [ref_train_iteration(model, opt, img, lab, zs[0:6]),
              ref_train_iteration(model, opt, img, lab, zs[6:12])]
    arrays['losses'] = np.array(losses, dtype=np.float64)
    fin = model.state_dict()
    for k in ['generator.blocks.2.conv.8.module.weight', 'generator.linear.module.bias',
              'discriminator.blocks.1.conv.2.module.weight_orig', 'discriminator.blocks.4.conv.5.module.weight_u'
              if 'discriminator.blocks.4.conv.5.module.weight_u' in fin else 'discriminator.blocks.3.conv.5.module.weight_u',
              'generator.blocks.3.module.running_var', 'discriminator.blocks.7.module.weight_orig']:
        arrays['digest/' + k] = gu.checksum(fin[k])
    save('mcgan_full_digest.npz', **arrays)


def fx_mcgan_coil():
    """Non-CIFAR block schedule (models/mcgan.py:166-175): G [64,32,16,8],
    D [8,16,32,64], 20 modes -- exercises channel-changing blocks and the
    stride-1 block with a 1x1 shortcut."""
    import models
    set_gan_cfg([64, 32, 16, 8], [8, 16, 32, 64], 20, data_name='COIL100')
    torch.manual_seed(5)
    model = models.mcgan()
    model.train(True)
    arrays = np_state(model.state_dict(), 'sd/')
    B = 4
    img, lab = gu.synthetic_batch(B, 20, seed=11)
    zs = gu.latent_batches(6, B, 128, seed=12)
    arrays['img'] = img.numpy(); arrays['label'] = lab.numpy(); arrays['z'] = torch.stack(zs).numpy()
    opt = make_opt(model)
    arrays['losses'] = np.array([ref_train_iteration(model, opt, img, lab, zs)], dtype=np.float64)
    arrays.update(np_state(model.state_dict(), 'sd_final/'))
    save('mcgan_coil_small.npz', **arrays)


FIXTURES = {'mc_unit': fx_mc_unit, 'blocks': fx_blocks, 'mcgan_small': fx_mcgan_small,
            'mcgan_full': fx_mcgan_full, 'mcgan_coil': fx_mcgan_coil}

def fx_dp_emulation():
    """Two-replica data parallel as the reference's nn.DataParallel computes it (train_gan.py:96-98):
    the same weights see two batch shards (per-shard BatchNorm statistics), gradients are averaged.
    Stored: the averaged gradients of one D loss and one G loss on the reduced-width model."""
    import models
    set_gan_cfg([32] * 4, [16] * 4, 10)
    torch.manual_seed(0)
    model = models.mcgan()
    model.train(True)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    B = 8
    img, lab = gu.synthetic_batch(B, 10, seed=21)
    z = gu.latent_batches(2, B, 128, seed=22)
    arrays = np_state(sd0, 'sd/')
    arrays['img'] = img.numpy(); arrays['label'] = lab.numpy(); arrays['z'] = torch.stack(z).numpy()
    shards = [slice(0, B // 2), slice(B // 2, B)]
    for step in ('d', 'g'):
        acc = None
        for sh in shards:
            model.load_state_dict(sd0)
            model.zero_grad()
            if step == 'd':
                d_x = model.discriminate(img[sh], lab[sh])
                fake = model.generate(lab[sh], z[0][sh])
                loss = F.relu(1.0 - d_x).mean() + F.relu(1.0 + model.discriminate(fake.detach(), lab[sh])).mean()
            else:
                loss = -model.discriminate(model.generate(lab[sh], z[1][sh]), lab[sh]).mean()
            loss.backward()
            net = model.discriminator if step == 'd' else model.generator
            g = {n: p.grad.clone() for n, p in net.named_parameters()}
            acc = g if acc is None else {n: acc[n] + g[n] for n in g}
        for n, v in acc.items():
            arrays[f'grad_{step}/{n}'] = (v / len(shards)).numpy()
    save('mcgan_dp2.npz', **arrays)


FIXTURES['dp'] = fx_dp_emulation

class _PatchedNoise:
    """Make torch.randn_like / torch.rand_like return (and record) tensors from a seeded CPU generator,
    so the noise the reference draws INSIDE its models becomes part of the fixture."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.drawn = []

    def __enter__(self):
        self._randn_like, self._rand_like = torch.randn_like, torch.rand_like
        torch.randn_like = lambda t, **k: self._draw(torch.randn(t.shape, generator=self.g))
        torch.rand_like = lambda t, **k: self._draw(torch.rand(t.shape, generator=self.g))
        return self

    def _draw(self, t):
        self.drawn.append(t.clone())
        return t

    def __exit__(self, *a):
        torch.randn_like, torch.rand_like = self._randn_like, self._rand_like


def _single_opt_steps(model, inputs, noise_seed, steps, arrays, clip=1.0, lr=3e-4):
    """train_vae.py:98-126 / train_glow.py / train_pixelcnn.py loop body: zero_grad, forward, backward,
    clip_grad_norm_(1), Adam(lr 3e-4).step()."""
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    losses = []
    for s in range(steps):
        with _PatchedNoise(noise_seed + s) as pn:
            opt.zero_grad()
            out = model({k: (v.clone() if torch.is_tensor(v) else v) for k, v in inputs.items()})
            out['loss'].backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
            opt.step()
        losses.append(out['loss'].item())
        for j, t in enumerate(pn.drawn):
            arrays[f'noise/{s}/{j}'] = t.numpy()
        if s == 0:
            first = out
    arrays['losses'] = np.array(losses, dtype=np.float64)
    return first


def fx_mcvae_small():
    """MCVAE (config 0 family), reduced width [8, 16, 32], latent 16, B=8, 3 optimizer steps."""
    import models
    cfg['model_name'] = 'mcvae'; cfg['data_name'] = 'CIFAR10'; cfg['device'] = 'cpu'; cfg['classes_size'] = 10
    cfg['controller_rate'] = 0.5; cfg['data_shape'] = [3, 32, 32]
    cfg['vae'] = {'hidden_size': [8, 16, 32], 'latent_size': 16, 'num_res_block': 2, 'embedding_size': 32}
    torch.manual_seed(0)
    model = models.mcvae(); model.train(True)
    arrays = np_state(model.state_dict(), 'sd/')
    img, lab = gu.synthetic_batch(8, 10, seed=31)
    arrays['img'] = img.numpy(); arrays['label'] = lab.numpy()
    first = _single_opt_steps(model, {'img': img, 'label': lab}, 100, 3, arrays)
    arrays['mu0'] = first['mu'].detach().numpy(); arrays['logvar0'] = first['logvar'].detach().numpy()
    arrays['img0'] = first['img'].detach().numpy()
    arrays.update(np_state(model.state_dict(), 'sd_final/'))
    model.train(False)
    z = torch.randn(8, 16, generator=torch.Generator().manual_seed(5))
    arrays['gen_z'] = z.numpy()
    with torch.no_grad():
        arrays['generated_eval'] = model.generate(lab, z).numpy()
    save('mcvae_small.npz', **arrays)


def fx_mcvae_full():
    """Config 0 of BASELINE.json: MCVAE CIFAR-10 (hidden [64,128,256], latent 128), batch 32, on CPU:
    losses of 2 optimizer steps + output digests; weights = the reference's own seed-0 init, stored."""
    import models
    cfg['model_name'] = 'mcvae'; cfg['data_name'] = 'CIFAR10'; cfg['device'] = 'cpu'; cfg['classes_size'] = 10
    cfg['controller_rate'] = 0.5; cfg['data_shape'] = [3, 32, 32]
    cfg['vae'] = {'hidden_size': [64, 128, 256], 'latent_size': 128, 'num_res_block': 2, 'embedding_size': 32}
    torch.manual_seed(0)
    model = models.mcvae(); model.train(True)
    assert sum(p.numel() for p in model.parameters()) == 7628931
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = gu.procedural_state_generic(shapes, seed=4321)
    model.load_state_dict(sd)
    arrays = {'shape_keys': np.array(sorted(shapes)), 'shape_vals': np.array([str(shapes[k]) for k in sorted(shapes)])}
    img, lab = gu.synthetic_batch(32, 10, seed=1)
    first = _single_opt_steps(model, {'img': img, 'label': lab}, 200, 2, arrays)
    arrays['mu0_digest'] = gu.checksum(first['mu']); arrays['img0_digest'] = gu.checksum(first['img'])
    arrays['img0_sample'] = first['img'].detach().numpy()[:4, :, ::4, ::4].copy()
    save('mcvae_full_digest.npz', **arrays)


def fx_mcpixelcnn_small():
    """MCGatedPixelCNN, hidden 16, 4 layers, 32 codes, 8x8 code maps, B=6, 3 optimizer steps."""
    import models
    cfg['model_name'] = 'mcpixelcnn'; cfg['device'] = 'cpu'; cfg['classes_size'] = 10; cfg['controller_rate'] = 0.5
    cfg['pixelcnn'] = {'num_layer': 4, 'hidden_size': 16, 'num_embedding': 32}
    torch.manual_seed(0)
    model = models.mcpixelcnn(); model.train(True)
    arrays = np_state(model.state_dict(), 'sd/')
    g = torch.Generator().manual_seed(41)
    codes = torch.randint(0, 32, (6, 8, 8), generator=g)
    lab = torch.randint(0, 10, (6,), generator=g)
    arrays['codes'] = codes.numpy(); arrays['label'] = lab.numpy()
    first = _single_opt_steps(model, {'img': codes, 'label': lab}, 300, 3, arrays)
    arrays['logits0'] = first['logits'].detach().numpy()
    arrays.update(np_state(model.state_dict(), 'sd_final/'))
    model.train(False)
    with torch.no_grad():
        arrays['logits_eval'] = model({'img': codes, 'label': lab})['logits'].numpy()
    save('mcpixelcnn_small.npz', **arrays)


def fx_mcglow_small():
    """MCGlow [1,32,32], K=2, L=3, hidden 32, 12 modes, B=4: ActNorm data init (first forward), 2 optimizer
    steps, reverse(reconstruct) and sampling from fixed z."""
    import models
    cfg['model_name'] = 'mcglow'; cfg['device'] = 'cpu'; cfg['classes_size'] = 12; cfg['controller_rate'] = 0.5
    cfg['data_shape'] = [1, 32, 32]
    cfg['glow'] = {'hidden_size': 32, 'K': 2, 'L': 3, 'affine': True, 'conv_lu': True}
    torch.manual_seed(0); np.random.seed(0)
    model = models.mcglow(); model.train(True)
    arrays = np_state(model.state_dict(), 'sd/')
    img, lab = gu.synthetic_batch(4, 12, seed=51, shape=(1, 32, 32))
    arrays['img'] = img.numpy(); arrays['label'] = lab.numpy()
    with _PatchedNoise(400) as pn, torch.no_grad():                       # train_glow.py:60-67 data-dependent init
        model({'img': img.clone(), 'label': lab})
    arrays['noise/init/0'] = pn.drawn[0].numpy()
    arrays.update(np_state(model.state_dict(), 'sd_init/'))
    first = _single_opt_steps(model, {'img': img, 'label': lab}, 500, 2, arrays)
    for i, z in enumerate(first['z']):
        arrays[f'z0/{i}'] = z.detach().numpy()
    arrays.update(np_state(model.state_dict(), 'sd_final/'))
    model.train(False)
    with torch.no_grad(), _PatchedNoise(600) as pn:
        out = model({'img': img.clone(), 'label': lab})
        arrays['noise/eval/0'] = pn.drawn[0].numpy()
        arrays['loss_eval'] = np.array(out['loss'].item())
        rec = model.reverse({'z': out['z'], 'label': lab, 'reconstruct': True})['img']
        arrays['reconstructed'] = rec.numpy()
        gz = [torch.randn(4, *s, generator=torch.Generator().manual_seed(7 + i)) * 0.7 for i, s in enumerate(model.make_z_shapes())]
        for i, z in enumerate(gz):
            arrays[f'gen_z/{i}'] = z.numpy()
        arrays['generated'] = model.generate(lab, gz).numpy()
    save('mcglow_small.npz', **arrays)


def fx_vqvae_small():
    """VQ-VAE (the frozen auto-encoder in front of MCPixelCNN, train_pixelcnn.py:111-113), reduced: hidden [16, 16],
    64 codes of size 8, B=4.  Two training-mode forwards move the BN running statistics and the EMA codebook off
    their initial values; then the eval-mode encode (encoder output, code map, quantised tensor) and decode_code."""
    import models
    cfg['model_name'] = 'vqvae'; cfg['device'] = 'cpu'; cfg['data_shape'] = [3, 32, 32]
    cfg['vqvae'] = {'hidden_size': [16, 16], 'num_res_block': 2, 'embedding_size': 8, 'num_embedding': 64, 'vq_commit': 0.25}
    torch.manual_seed(0)
    model = models.vqvae(); model.train(True)
    img, _ = gu.synthetic_batch(4, 10, seed=61)
    with torch.no_grad():
        for _ in range(2):
            model({'img': img.clone()})
    model.train(False)
    with torch.no_grad():
        # a random-init encoder maps everything next to one code; spread the codebook over the encoder's outputs
        # (the codebook is state, i.e. an input of this fixture) so that the arg-min is exercised
        flat0 = model.encoder(img).transpose(1, -1).contiguous().view(-1, 8)
        gsel = torch.Generator().manual_seed(62)
        model.quantizer.embedding.copy_((flat0[::4] + 0.02 * torch.randn(64, 8, generator=gsel)).t())
    arrays = np_state(model.state_dict(), 'sd/')
    arrays['img'] = img.numpy()
    with torch.no_grad():
        x = model.encoder(img)
        encoded, vq_loss, code = model.encode(img)
        arrays['enc_out'] = x.numpy(); arrays['encoded'] = encoded.numpy(); arrays['code'] = code.numpy()
        arrays['vq_loss'] = np.array(vq_loss.item())
        arrays['decoded'] = model.decode_code(code).numpy()
        flat = x.transpose(1, -1).contiguous().view(-1, 8)
        emb = model.quantizer.embedding
        dist = flat.pow(2).sum(1, keepdim=True) - 2 * flat @ emb + emb.pow(2).sum(0, keepdim=True)
        top2 = dist.topk(2, dim=1, largest=False).values
        arrays['dist_margin'] = (top2[:, 1] - top2[:, 0]).numpy()          # how decisive each argmin is
    save('vqvae_small.npz', **arrays)


FIXTURES.update(vqvae=fx_vqvae_small)
FIXTURES.update(mcvae_small=fx_mcvae_small, mcvae_full=fx_mcvae_full, mcpixelcnn=fx_mcpixelcnn_small, mcglow=fx_mcglow_small)


def _hook_checksums(model, arrays, tag):
    """Forward hooks on every top-level block of G and D: order-sensitive checksums of the block outputs
    (NCHW, as the reference holds them) of the NEXT forward of each network."""
    handles = []
    for net_name in ('generator', 'discriminator'):
        net = getattr(model, net_name)
        for i, blk in enumerate(net.blocks.children()):
            def hook(mod, inp, out, key=f'{tag}/{net_name}.blocks.{i}'):
                t = out[0] if isinstance(out, (list, tuple)) else out
                if torch.is_tensor(t) and t.dim() == 4 and key not in arrays:
                    arrays[key] = gu.checksum(t)
            handles.append(blk.register_forward_hook(hook))
    return handles


def fx_mcgan_full_b128():
    """BASELINE configs[1] at its stated batch: full-size MCGAN (utils.py:156-162), procedural weights, B=128,
    ONE train iteration (train_gan.py:139-176): losses, a strided sample + digest of the probe batch, per-block
    activation digests of one G and one D forward, digests of a few final tensors."""
    import models
    g_hidden, d_hidden = [256] * 4, [128] * 4
    set_gan_cfg(g_hidden, d_hidden, 10)
    torch.manual_seed(0)
    model = models.mcgan()
    sd = gu.procedural_state(gu.mcgan_shapes(g_hidden, d_hidden, 10), seed=1234, num_mode=10)
    model.load_state_dict(sd)
    model.train(True)
    B = 128
    img, lab = gu.synthetic_batch(B, 10, seed=1)
    zs = gu.latent_batches(6, B, 128, seed=2)
    arrays = {}
    hs = _hook_checksums(model, arrays, 'act')
    with torch.no_grad():
        gen0 = model.generate(lab, zs[0])
        d0 = model.discriminate(img, lab)
    for h in hs:
        h.remove()
    arrays['probe_generated'] = gen0.numpy()[:, :, ::4, ::4].copy()
    arrays['probe_generated_digest'] = gu.checksum(gen0)
    arrays['probe_d_real'] = d0.numpy()
    model.load_state_dict(sd)
    opt = make_opt(model)
    arrays['losses'] = np.array([ref_train_iteration(model, opt, img, lab, zs)], dtype=np.float64)
    fin = model.state_dict()
    for k in ['generator.blocks.2.conv.8.module.weight', 'generator.blocks.1.conv.4.module.weight', 'generator.linear.module.bias',
              'discriminator.blocks.0.conv.3.module.weight_orig', 'discriminator.blocks.1.conv.2.module.weight_orig',
              'discriminator.blocks.3.conv.5.module.weight_u', 'generator.blocks.3.module.running_var',
              'generator.blocks.2.conv.5.module.running_mean']:
        arrays['digest/' + k] = gu.checksum(fin[k])
    save('mcgan_full_digest_b128.npz', **arrays)


def fx_mcgan_coil_full():
    """BASELINE configs[2] as the reference runs it (utils.py:116-118,163-165; data.py:51): COIL100 at 32x32,
    G [512,256,128,64], D [64,128,256,512], 100 modes, non-CIFAR block schedule; procedural weights, B=8,
    one train iteration + probes."""
    import models
    g_hidden, d_hidden = [512, 256, 128, 64], [64, 128, 256, 512]
    set_gan_cfg(g_hidden, d_hidden, 100, data_name='COIL100')
    torch.manual_seed(0)
    model = models.mcgan()
    shapes = gu.mcgan_shapes(g_hidden, d_hidden, 100, cifar_layout=False)
    ref_shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert shapes == ref_shapes, set(shapes.items()) ^ set(ref_shapes.items())
    sd = gu.procedural_state(shapes, seed=4242, num_mode=100)
    model.load_state_dict(sd)
    model.train(True)
    B = 8
    img, lab = gu.synthetic_batch(B, 100, seed=5)
    zs = gu.latent_batches(6, B, 128, seed=6)
    arrays = {}
    hs = _hook_checksums(model, arrays, 'act')
    with torch.no_grad():
        gen0 = model.generate(lab, zs[0])
        d0 = model.discriminate(img, lab)
    for h in hs:
        h.remove()
    arrays['probe_generated'] = gen0.numpy().copy()
    arrays['probe_d_real'] = d0.numpy()
    model.load_state_dict(sd)
    opt = make_opt(model)
    arrays['losses'] = np.array([ref_train_iteration(model, opt, img, lab, zs)], dtype=np.float64)
    fin = model.state_dict()
    for k in ['generator.blocks.0.conv.4.module.weight', 'generator.blocks.2.shortcut.2.module.weight',
              'discriminator.blocks.3.conv.5.module.weight_orig', 'discriminator.blocks.2.shortcut.1.module.weight_u']:
        arrays['digest/' + k] = gu.checksum(fin[k])
    save('mcgan_coil_full_digest.npz', **arrays)


def fx_mcglow_full():
    """BASELINE configs[3] as the reference runs it (utils.py:110-112,172-184; data.py:40): MCGlow on Omniglot
    [1,32,32], 1623 modes, hidden 512, K=16, L=3 (15,844,992 parameters); procedural weights (golden_util.
    procedural_state_glow), B=4: ActNorm data init forward, then two train_glow.py steps; losses + z digests."""
    import models
    cfg['model_name'] = 'mcglow'; cfg['device'] = 'cpu'; cfg['classes_size'] = 1623; cfg['controller_rate'] = 0.5
    cfg['data_shape'] = [1, 32, 32]
    cfg['glow'] = {'hidden_size': 512, 'K': 16, 'L': 3, 'affine': True, 'conv_lu': True}
    torch.manual_seed(0); np.random.seed(0)
    model = models.mcglow(); model.train(True)
    assert sum(p.numel() for p in model.parameters()) == 15844992
    ref_sd = model.state_dict()
    keys = sorted(ref_sd)
    shapes = {k: tuple(ref_sd[k].shape) for k in keys}
    dtypes = {k: str(ref_sd[k].dtype).replace('torch.', '') for k in keys}
    sd = gu.procedural_state_glow(shapes, dtypes, seed=777)
    model.load_state_dict(sd)
    arrays = {'shape_keys': np.array(keys), 'shape_vals': np.array([str(shapes[k]) for k in keys]),
              'dtype_vals': np.array([dtypes[k] for k in keys])}
    img, lab = gu.synthetic_batch(4, 1623, seed=71, shape=(1, 32, 32))
    arrays['img'] = img.numpy(); arrays['label'] = lab.numpy()
    with _PatchedNoise(800) as pn, torch.no_grad():                       # train_glow.py:60-67 data-dependent init
        model({'img': img.clone(), 'label': lab})
    arrays['noise/init/0'] = pn.drawn[0].numpy()
    init = model.state_dict()
    for k in ['blocks.0.flows.0.actnorm.loc', 'blocks.0.flows.0.coupling.net.1.module.scale',
              'blocks.1.flows.7.coupling.net.5.module.loc', 'blocks.2.flows.15.actnorm.scale']:
        arrays['init_digest/' + k] = gu.checksum(init[k])
    first = _single_opt_steps(model, {'img': img, 'label': lab}, 900, 2, arrays)
    for i, z in enumerate(first['z']):
        arrays[f'z0_digest/{i}'] = gu.checksum(z)
        arrays[f'z0_sample/{i}'] = z.detach().numpy()[:, :, ::2, ::2].copy()
    fin = model.state_dict()
    for k in ['blocks.0.flows.3.coupling.net.4.module.weight', 'blocks.2.flows.9.invconv.w_l', 'blocks.1.prior.conv.weight']:
        arrays['final_digest/' + k] = gu.checksum(fin[k])
    save('mcglow_full_digest.npz', **arrays)


def fx_mcpixelcnn_full():
    """BASELINE configs[4] as the reference runs it (utils.py:139-143): MCGatedPixelCNN with 15 layers, hidden 128,
    512 codes, 10 modes (6,367,616 parameters) on 8x8 code maps at the config's batch 128; procedural weights
    (golden_util.procedural_state_generic).  Loss + logits digest of the first training forward, the digest of EVERY
    parameter's gradient of that step (before clip_grad_norm_), two train_pixelcnn.py steps (losses), digests of a few
    final tensors -- a key that is absent from the state dict is an error, not a silent skip."""
    import models
    cfg['model_name'] = 'mcpixelcnn'; cfg['device'] = 'cpu'; cfg['classes_size'] = 10; cfg['controller_rate'] = 0.5
    cfg['pixelcnn'] = {'num_layer': 15, 'hidden_size': 128, 'num_embedding': 512}
    torch.manual_seed(0)
    model = models.mcpixelcnn(); model.train(True)
    assert sum(p.numel() for p in model.parameters()) == 6367616
    ref_sd = model.state_dict()
    keys = sorted(ref_sd)
    shapes = {k: tuple(ref_sd[k].shape) for k in keys}
    model.load_state_dict(gu.procedural_state_generic(shapes, seed=4242))
    arrays = {'shape_keys': np.array(keys), 'shape_vals': np.array([str(shapes[k]) for k in keys])}
    g = torch.Generator().manual_seed(43)
    B = 128
    codes = torch.randint(0, 512, (B, 8, 8), generator=g)
    lab = torch.randint(0, 10, (B,), generator=g)
    arrays['codes'] = codes.numpy(); arrays['label'] = lab.numpy()
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)                           # train_pixelcnn.py:33,108-121
    losses = []
    for step in range(2):
        opt.zero_grad()
        out = model({'img': codes.clone(), 'label': lab})
        out['loss'].backward()
        if step == 0:
            arrays['logits0_digest'] = gu.checksum(out['logits'].detach())
            arrays['logits0_sample'] = out['logits'].detach().numpy()[::16, ::16, ::2, ::2].copy()
            names, dead = [], []
            for k, p in model.named_parameters():
                if p.grad is None:                       # (the last layer's vertical stream feeds nothing: mcpixelcnn.py:56-61)
                    dead.append(k)
                    continue
                names.append(k)
                arrays['grad0_digest/' + k] = gu.checksum(p.grad)
                arrays['grad0_absmax/' + k] = np.array(float(p.grad.abs().max()))
            arrays['grad_keys'] = np.array(names)
            arrays['nograd_keys'] = np.array(dead)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1)
        opt.step()
        losses.append(out['loss'].item())
    arrays['losses'] = np.array(losses, dtype=np.float64)
    fin = model.state_dict()
    final = ['layers.0.vert_stack.weight', 'layers.7.horiz_resid.0.module.weight', 'layers.14.gate_h.bn.running_var', 'output_conv.4.module.weight']
    for k in final:
        if k not in fin:
            raise KeyError(f'{k} is not a key of the reference state dict (have e.g. {[x for x in fin if x.startswith(k.split(".")[0])][:8]})')
        arrays['final_digest/' + k] = gu.checksum(fin[k].float())
    arrays['final_keys'] = np.array(final)
    save('mcpixelcnn_full_digest.npz', **arrays)


def fx_classifier():
    """The feature network of IS / FID on COIL100 / Omniglot (models/classifier.py:14-52; metrics.py:49-62,89-113):
    hidden [8, 16, 32, 64] (utils.py:185), evaluation mode, on both data shapes ([3,32,32] and Omniglot's [1,32,32]); weights from the reference's own
    initialisation with non-trivial BatchNorm running statistics.  Outputs: features and logits of a batch, and the
    Inception Score / FID the reference's formulas (metrics.py:75-82,139-161) give on them."""
    import models
    from scipy import linalg
    arrays = {}
    for tag, shape, classes in (('coil100', [3, 32, 32], 100), ('gray', [1, 32, 32], 40)):     # (Omniglot's shape; 40 of its 1623 classes keep the file small)
        cfg['model_name'] = 'classifier'; cfg['device'] = 'cpu'; cfg['classes_size'] = classes; cfg['data_shape'] = shape
        cfg['classifier'] = {'hidden_size': [8, 16, 32, 64]}
        torch.manual_seed(5)
        model = models.classifier()
        g = torch.Generator().manual_seed(61)
        with torch.no_grad():
            for m in model.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                    m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
        model.train(False)
        arrays.update(np_state(model.state_dict(), f'{tag}/sd/'))
        img = torch.rand(20, *shape, generator=g) * 2 - 1
        real = torch.rand(24, *shape, generator=g) * 2 - 1
        arrays[f'{tag}/img'] = img.numpy(); arrays[f'{tag}/real'] = real.numpy()
        with torch.no_grad():
            feat = model.feature({'img': img})
            out = model({'img': img, 'label': torch.zeros(20, dtype=torch.long)})
            rfeat = model.feature({'img': real})
        arrays[f'{tag}/feature'] = feat.numpy(); arrays[f'{tag}/logits'] = out['label'].numpy()
        pred = F.softmax(out['label'], dim=-1)                                    # metrics.py:61-62,75-81
        py = pred.mean(0)
        arrays[f'{tag}/inception_score'] = np.array(F.kl_div(py.log().view(1, -1).expand_as(pred), pred, reduction='batchmean').exp().item())
        a, b = rfeat.numpy().astype(np.float64), feat.numpy().astype(np.float64)  # metrics.py:139-161
        mu1, mu2 = a.mean(0), b.mean(0)
        s1, s2 = np.cov(a, rowvar=False), np.cov(b, rowvar=False)
        covmean, _ = linalg.sqrtm(s1.dot(s2), disp=False)
        if not np.isfinite(covmean).all():
            off = np.eye(s1.shape[0]) * 1e-6
            covmean = linalg.sqrtm((s1 + off).dot(s2 + off))
        covmean = covmean.real if np.iscomplexobj(covmean) else covmean
        d = mu1 - mu2
        arrays[f'{tag}/fid'] = np.array(d.dot(d) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean))
    save('classifier_small.npz', **arrays)


FIXTURES.update(mcgan_full_b128=fx_mcgan_full_b128, mcgan_coil_full=fx_mcgan_coil_full, mcglow_full=fx_mcglow_full,
                mcpixelcnn_full=fx_mcpixelcnn_full, classifier=fx_classifier)

def _vqvae_steps(model, img, steps, arrays, clip=1.0, lr=3e-4):
    """train_vqvae.py:99-112 loop body (zero_grad, forward, backward, clip_grad_norm_(1), Adam(lr 3e-4).step()).
    Step 0 also records the quantiser's input / codebook before its update and the MSE / VQ parts of the loss, every
    parameter's gradient before clipping and every buffer after the step."""
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    seen = {}

    def pre(mod, inp):
        seen['x'] = inp[0].detach().clone(); seen['emb'] = mod.embedding.clone()

    def post(mod, inp, out):
        seen['diff'] = out[1].detach().clone()
    h1 = model.quantizer.register_forward_pre_hook(pre)
    h2 = model.quantizer.register_forward_hook(post)
    losses, first = [], None
    for s in range(steps):
        opt.zero_grad()
        out = model({'img': img.clone()})
        out['loss'].backward()
        if s == 0:
            first = dict(out, x=seen['x'], emb=seen['emb'], diff=seen['diff'],
                         grads={k: p.grad.detach().clone() for k, p in model.named_parameters()})
        torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        opt.step()
        if s == 0:
            first['buffers'] = {k: b.detach().clone() for k, b in model.named_buffers()}
        losses.append(out['loss'].item())
    h1.remove(); h2.remove()
    arrays['losses'] = np.array(losses, dtype=np.float64)
    return first


def _vq_margin(x, emb):
    d = emb.shape[0]
    flat = x.transpose(1, -1).contiguous().view(-1, d)
    dist = flat.pow(2).sum(1, keepdim=True) - 2 * flat @ emb + emb.pow(2).sum(0, keepdim=True)
    top2 = dist.topk(2, dim=1, largest=False).values
    return (top2[:, 1] - top2[:, 0]).view(*x.transpose(1, -1).shape[:-1])


def _set_vqvae_cfg(hidden, d, k):
    cfg['model_name'] = 'vqvae'; cfg['device'] = 'cpu'; cfg['data_shape'] = [3, 32, 32]
    cfg['vqvae'] = {'hidden_size': list(hidden), 'num_res_block': 2, 'embedding_size': d, 'num_embedding': k, 'vq_commit': 0.25}


def fx_vqvae_train_small():
    """VQ-VAE training (train_vqvae.py:99-112), reduced: hidden [16, 16], 2 res blocks, D 8, K 64, B 8.  The codebook
    (embedding = embedding_mean) is spread over the initial training-mode encoder outputs so that many codes are hit.
    Step 0 in detail (loss parts, code map + arg-min margin, decoded image, gradients before clipping, buffers after),
    the losses of 3 loop-body steps, the final state and an eval-mode forward on it."""
    import models
    _set_vqvae_cfg([16, 16], 8, 64)
    torch.manual_seed(0)
    model = models.vqvae(); model.train(True)
    img, _ = gu.synthetic_batch(8, 10, seed=71)
    with torch.no_grad():
        keep = {k: v.clone() for k, v in model.state_dict().items()}
        flat0 = model.encoder(img).transpose(1, -1).contiguous().view(-1, 8)
        model.load_state_dict(keep)                     # (undo the BN running-statistics update of that probe)
        gsel = torch.Generator().manual_seed(72)
        emb = (flat0[::8] + 0.02 * torch.randn(64, 8, generator=gsel)).t().contiguous()
        model.quantizer.embedding.copy_(emb); model.quantizer.embedding_mean.copy_(emb)
    arrays = np_state(model.state_dict(), 'sd/')
    arrays['img'] = img.numpy()
    first = _vqvae_steps(model, img, 3, arrays)
    arrays['loss0'] = np.array(first['loss'].item())
    arrays['mse0'] = np.array(F.mse_loss(first['img'], img).item())
    arrays['vq0'] = np.array(first['diff'].item())
    arrays['code0'] = first['code'].numpy()
    arrays['dist_margin0'] = _vq_margin(first['x'], first['emb']).numpy()
    arrays['img0'] = first['img'].detach().numpy()
    for k, g in first['grads'].items():
        arrays['grad0/' + k] = g.numpy()
    for k, b in first['buffers'].items():
        arrays['buf1/' + k] = b.numpy()
    arrays.update(np_state(model.state_dict(), 'sd_final/'))
    model.train(False)
    with torch.no_grad():
        out = model({'img': img.clone()})
    arrays['eval_loss'] = np.array(out['loss'].item())
    arrays['eval_code'] = out['code'].numpy()
    save('vqvae_train_small.npz', **arrays)


def fx_vqvae_train_full():
    """The shipped VQ-VAE (hidden [128, 128], D 64, K 512) at B = 128, 2 loop-body steps.  Weights: procedural stand-ins
    (gu.procedural_state_generic, seed 7301) with the quantiser's reference initialisation (embedding = embedding_mean
    ~ N(0, 1), stored; cluster_size 0), under which most pixels of the first step pick one code.  Recorded: the losses,
    the step-0 code histogram, per-parameter gradient norms before clipping, a strided slice of the decoded image and
    cluster_size / embedding after step 0."""
    import models
    _set_vqvae_cfg([128, 128], 64, 512)
    torch.manual_seed(0)
    model = models.vqvae(); model.train(True)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = gu.procedural_state_generic(shapes, seed=7301)
    emb = torch.randn(64, 512, generator=torch.Generator().manual_seed(7302))
    sd['quantizer.embedding'] = emb.clone(); sd['quantizer.embedding_mean'] = emb.clone()
    sd['quantizer.cluster_size'] = torch.zeros(512)
    model.load_state_dict(sd)
    arrays = {'q_embedding': emb.numpy()}
    img, _ = gu.synthetic_batch(128, 10, seed=73)
    first = _vqvae_steps(model, img, 2, arrays)
    arrays['hist0'] = torch.bincount(first['code'].flatten(), minlength=512).numpy()
    names = sorted(first['grads'])
    arrays['grad_names'] = np.array(names)
    arrays['grad_norms'] = np.array([first['grads'][k].double().norm().item() for k in names])
    arrays['img0_sample'] = first['img'].detach().numpy()[:4, :, ::4, ::4].copy()
    arrays['cluster_size1'] = first['buffers']['quantizer.cluster_size'].numpy()
    arrays['embedding1'] = first['buffers']['quantizer.embedding'].numpy()
    arrays['vq0'] = np.array(first['diff'].item())
    save('vqvae_train_full_digest.npz', **arrays)


FIXTURES.update(vqvae_train_small=fx_vqvae_train_small, vqvae_train_full=fx_vqvae_train_full)


def _set_classifier_cfg(shape, classes):
    cfg['model_name'] = 'classifier'; cfg['device'] = 'cpu'; cfg['classes_size'] = classes; cfg['data_shape'] = list(shape)
    cfg['classifier'] = {'hidden_size': [8, 16, 32, 64]}


def _classifier_steps(model, img, label, steps, lr=1e-2, clip=1.0):
    """train_classifier.py:104-113 loop body: zero_grad, training-mode forward, backward, clip_grad_norm_(1), Adam(lr 1e-2,
    weight_decay 0).step().  -> (losses, logits per step, step-1 gradients before clipping)."""
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0)
    model.train(True)
    losses, logits, grads = [], [], None
    for s in range(steps):
        opt.zero_grad()
        out = model({'img': img.clone(), 'label': label.clone()})
        out['loss'].backward()
        if s == 0:
            grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
        torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
        opt.step()
        losses.append(out['loss'].item()); logits.append(out['label'].detach().clone())
    return losses, logits, grads


def _classifier_margin(model, img):
    """Smallest distance, relative to the per-channel spread, between the two largest ReLU outputs of a max-pool window
    (the larger one > 0) and of any BatchNorm output from 0, over the fp64 training-mode forward of `img`.  A near-tie
    or a near-zero there makes the gradient's routing depend on rounding, so the fixtures pick inputs that keep a margin."""
    convs = [m for m in model.blocks if isinstance(m, torch.nn.Conv2d)]
    bns = [m for m in model.blocks if isinstance(m, torch.nn.BatchNorm2d)]
    x, margin = img.double(), float('inf')
    with torch.no_grad():
        for i, (conv, bn) in enumerate(zip(convs, bns)):
            x = F.conv2d(x, conv.weight.double(), conv.bias.double(), padding=1)
            z = F.batch_norm(x, None, None, bn.weight.double(), bn.bias.double(), training=True, eps=bn.eps)
            spread = z.std((0, 2, 3), keepdim=True)
            margin = min(margin, float((z.abs() / spread).min()))
            x = F.relu(z)
            if i + 1 < len(convs):
                n, c, h, w = x.shape
                win = (x / spread).view(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
                top = win.topk(2, -1).values
                live = top[..., 0] > 0
                if live.any():
                    margin = min(margin, float((top[..., 0] - top[..., 1])[live].min()))
                x = F.max_pool2d(x, 2)
    return margin


def _classifier_inputs(model, n, shape, classes, seed, need):
    """The first input seed from `seed` on whose batch keeps _classifier_margin >= need."""
    for s in range(seed, seed + 1000):
        img, label = gu.synthetic_batch(n, classes, seed=s, shape=tuple(shape))
        if _classifier_margin(model, img) >= need:
            return s, img, label
    raise RuntimeError('no input seed with the requested margin')


CLASSIFIER_SMALL = (('coil100', [3, 32, 32], 100, 7411), ('gray', [1, 32, 32], 16, 7412))


def fx_classifier_train_small():
    """Classifier training (train_classifier.py:104-113) at B = 16 for 3 steps on both data shapes: COIL100 [3,32,32] with
    100 classes and Omniglot's [1,32,32] (16 of its 1623 classes keep the file small; the 1623-class head is in the digest).
    The initial weights (gu.procedural_state_generic, seed 7411 / 7412) and the inputs (gu.synthetic_batch: for the training
    batch the first seed from seed + 100 on that keeps a routing margin of 3e-6, stored as input_seed; seed + 200 for the
    feature batch) are regenerated by the tests, so only results are stored: per-step
    loss and logits, step-1 gradients, the state after step 3 (BatchNorm buffers included; of the head weight every
    fourth row) and an eval-mode feature() of the feature batch on it."""
    import models
    arrays = {}
    for tag, shape, classes, seed in CLASSIFIER_SMALL:
        _set_classifier_cfg(shape, classes)
        torch.manual_seed(0)
        model = models.classifier()
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict(gu.procedural_state_generic(shapes, seed=seed))
        iseed, img, label = _classifier_inputs(model, 16, shape, classes, seed + 100, 3e-6)
        feat_img, _ = gu.synthetic_batch(12, classes, seed=seed + 200, shape=tuple(shape))
        losses, logits, grads = _classifier_steps(model, img, label, 3)
        arrays[f'{tag}/input_seed'] = np.array(iseed)
        arrays[f'{tag}/losses'] = np.array(losses, dtype=np.float64)
        arrays[f'{tag}/logits'] = torch.stack(logits).numpy()
        for k, g in grads.items():
            arrays[f'{tag}/grad1/{k}'] = g.numpy()
        arrays.update(np_state(model.state_dict(), f'{tag}/sd_final/'))
        arrays[f'{tag}/sd_final/classifier.weight'] = arrays[f'{tag}/sd_final/classifier.weight'][::4].copy()     # (size)
        model.train(False)
        with torch.no_grad():
            arrays[f'{tag}/feature'] = model.feature({'img': feat_img}).numpy()
    save('classifier_train_small.npz', **arrays)


def fx_classifier_train_full():
    """B = 128, both data shapes with their full class counts (COIL100 100, Omniglot 1623).  Weights: procedural stand-ins
    (gu.procedural_state_generic, seed 7401 / 7402); inputs gu.synthetic_batch from seed 83 / 84 on, the first with a
    routing margin of 2e-6 (_classifier_margin; stored as input_seed).  Recorded: per-parameter
    norms and sums of the step-1 gradients (before clipping) and the losses of 2 loop-body steps."""
    import models
    arrays = {}
    for tag, shape, classes, seed in (('coil100', [3, 32, 32], 100, 7401), ('omniglot', [1, 32, 32], 1623, 7402)):
        _set_classifier_cfg(shape, classes)
        torch.manual_seed(0)
        model = models.classifier()
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict(gu.procedural_state_generic(shapes, seed=seed))
        iseed, img, label = _classifier_inputs(model, 128, shape, classes, seed - 7318, 2e-6)
        losses, _, grads = _classifier_steps(model, img, label, 2)
        arrays[f'{tag}/input_seed'] = np.array(iseed)
        names = sorted(grads)
        arrays[f'{tag}/grad_names'] = np.array(names)
        arrays[f'{tag}/grad_norms'] = np.array([grads[k].double().norm().item() for k in names])
        arrays[f'{tag}/grad_sums'] = np.array([grads[k].double().sum().item() for k in names])
        arrays[f'{tag}/losses'] = np.array(losses, dtype=np.float64)
    save('classifier_train_full_digest.npz', **arrays)


FIXTURES.update(classifier_train_small=fx_classifier_train_small, classifier_train_full=fx_classifier_train_full)


# ---- CGAN (models/cgan.py): the conditional baseline, label embeddings instead of MultimodalControllers ---------------
def _set_cgan_cfg(g_hidden, d_hidden, classes, data_name='CIFAR10', channels=3):
    set_gan_cfg(g_hidden, d_hidden, classes, data_name)
    cfg['model_name'] = 'cgan'
    cfg['data_shape'] = [channels, 32, 32]


def _cgan_layout(shapes):
    """The reference's state_dict layout as one string array: 'key:d0xd1x...' per entry, in state_dict order."""
    return np.array([f"{k}:{'x'.join(str(d) for d in shp)}" for k, shp in shapes.items()])


def _cgan_small(name, data_name, channels, classes, iters, full_final=True):
    """Reduced-width CGAN on procedural weights (gu.procedural_state_generic over the reference's own state_dict layout,
    which is stored), `iters` train iterations at B=8: per-iteration losses, probes, the eval-mode generated batch and
    the state after training -- as its difference from the initial state (float16 for the >= 2-d weights, whose
    differences are a few Adam steps; float32 otherwise), or (`full_final` False) as digests only."""
    import models
    _set_cgan_cfg([32] * 4, [16] * 4, classes, data_name, channels)
    torch.manual_seed(0)
    model = models.cgan()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    seed = 4321
    sd0 = gu.procedural_state_generic(shapes, seed=seed)
    model.load_state_dict(sd0)
    model.train(True)
    arrays = {'layout': _cgan_layout(shapes), 'sd_seed': np.array(seed)}
    B = 8
    img, lab = gu.synthetic_batch(B, classes, seed=1, shape=(channels, 32, 32))
    if classes > B:
        lab[1] = lab[0]                                      # a repeated label among mostly distinct ones
    zs = gu.latent_batches(6 * iters + 1, B, 128, seed=2)
    arrays['img'] = img.numpy(); arrays['label'] = lab.numpy()
    arrays['z'] = torch.stack(zs).numpy()
    arrays['probe_generated'] = model.generate(lab, zs[-1]).detach().numpy()
    arrays['probe_d_real'] = model.discriminate(img, lab).detach().numpy()
    model.load_state_dict(sd0)
    opt = make_opt(model)
    losses = []
    for it in range(iters):
        losses.append(ref_train_iteration(model, opt, img, lab, zs[6 * it:6 * it + 6]))
    arrays['losses'] = np.array(losses, dtype=np.float64)
    fin = model.state_dict()
    for k, v in fin.items():
        if not v.is_floating_point():
            arrays['sd_final_int/' + k] = v.numpy().copy()
        elif full_final:
            dv = (v - sd0[k]).detach().numpy()
            arrays['sd_delta/' + k] = dv.astype(np.float16) if v.dim() >= 2 else dv
        else:
            arrays['digest/' + k] = gu.checksum(v)
    model.train(False)
    with torch.no_grad():
        arrays['final_generated_eval'] = model.generate(lab, zs[-1]).numpy()
        arrays['final_d_eval'] = model.discriminate(img, lab).numpy()
    save(name, **arrays)


def fx_cgan_small():
    _cgan_small('cgan_small.npz', 'CIFAR10', 3, 10, 2)


def fx_cgan_omniglot_small():
    _cgan_small('cgan_omniglot_small.npz', 'Omniglot', 1, 1623, 1, full_final=False)


def fx_cgan_full():
    """The CIFAR10 CGAN (utils.py:156-162 sizes) at batch 128 with procedural weights: probes, one train iteration's
    losses and digests of the state after it."""
    import models
    g_hidden, d_hidden = [256] * 4, [128] * 4
    _set_cgan_cfg(g_hidden, d_hidden, 10)
    torch.manual_seed(0)
    model = models.cgan()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = gu.procedural_state_generic(shapes, seed=1234)
    model.load_state_dict(sd)
    model.train(True)
    B = 128
    img, lab = gu.synthetic_batch(B, 10, seed=1)
    zs = gu.latent_batches(6, B, 128, seed=2)
    arrays = {'sd_seed': np.array(1234)}
    gen0 = model.generate(lab, zs[0])
    d0 = model.discriminate(img, lab)
    arrays['probe_generated_digest'] = gu.checksum(gen0)
    arrays['probe_generated'] = gen0.detach().numpy()[:16, :, ::4, ::4].copy()
    arrays['probe_d_real'] = d0.detach().numpy()
    model.load_state_dict(sd)
    opt = make_opt(model)
    arrays['losses'] = np.array([ref_train_iteration(model, opt, img, lab, zs)], dtype=np.float64)
    fin = model.state_dict()
    for k in ['generator.embedding.weight', 'generator.linear.weight', 'generator.blocks.2.conv.6.weight',
              'generator.blocks.3.running_var', 'discriminator.embedding.weight_orig', 'discriminator.embedding.weight_u',
              'discriminator.blocks.0.conv.0.weight_orig', 'discriminator.blocks.1.conv.3.weight_orig',
              'discriminator.blocks.6.weight_orig']:
        arrays['digest/' + k] = gu.checksum(fin[k])
    save('cgan_full_digest.npz', **arrays)


FIXTURES.update(cgan_small=fx_cgan_small, cgan_omniglot_small=fx_cgan_omniglot_small, cgan_full=fx_cgan_full)


# ---- CPixelCNN (models/cpixelcnn.py): the conditional PixelCNN baseline, per-layer label embeddings -------------------
def _set_cpixelcnn_cfg(hidden, layers, codes, classes):
    cfg['model_name'] = 'cpixelcnn'; cfg['device'] = 'cpu'; cfg['classes_size'] = classes
    cfg['pixelcnn'] = {'num_layer': layers, 'hidden_size': hidden, 'num_embedding': codes}


def _cpixelcnn_small(name, classes, full_final):
    """Hidden 16, 4 layers, 32 codes on 8x8 maps, B=6, procedural weights over the reference's layout (stored), 3
    train_pixelcnn.py steps: logits of the first forward, the losses, the state after training (differences from the
    initial state, or digests only), eval-mode logits of the trained model and its greedy decode (argmax per position
    through reference forwards, cpixelcnn.py:100-108 with the draw replaced)."""
    import models
    _set_cpixelcnn_cfg(16, 4, 32, classes)
    torch.manual_seed(0)
    model = models.cpixelcnn()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    seed = 2468
    sd0 = gu.procedural_state_generic(shapes, seed=seed)
    model.load_state_dict(sd0)
    model.train(True)
    arrays = {'layout': _cgan_layout(shapes), 'sd_seed': np.array(seed)}
    g = torch.Generator().manual_seed(47)
    codes = torch.randint(0, 32, (6, 8, 8), generator=g)
    lab = torch.randint(0, classes, (6,), generator=g)
    lab[1] = lab[0]                                          # a repeated label; with 6 samples most modes are absent
    lab[2] = classes - 1
    arrays['codes'] = codes.numpy(); arrays['label'] = lab.numpy()
    first = _single_opt_steps(model, {'img': codes, 'label': lab}, 500, 3, arrays)
    arrays['logits0'] = first['logits'].detach().numpy()
    fin = model.state_dict()
    for k, v in fin.items():
        if not v.is_floating_point():
            arrays['sd_final_int/' + k] = v.numpy().copy()
        elif full_final:
            arrays['sd_delta/' + k] = (v - sd0[k]).detach().numpy()
        else:
            arrays['digest/' + k] = gu.checksum(v)
    model.train(False)
    with torch.no_grad():
        arrays['logits_eval'] = model({'img': codes, 'label': lab})['logits'].numpy()
        x = torch.zeros((6, 8, 8), dtype=torch.long)
        for i in range(8):
            for j in range(8):
                out = model({'img': x, 'label': lab})
                x[:, i, j] = out['logits'][:, :, i, j].argmax(1)
        arrays['greedy'] = x.numpy()
    save(name, **arrays)


def fx_cpixelcnn_small():
    _cpixelcnn_small('cpixelcnn_small.npz', 10, True)


def fx_cpixelcnn_omniglot_small():
    _cpixelcnn_small('cpixelcnn_omniglot_small.npz', 1623, False)


def fx_cpixelcnn_full():
    """configs[4] shapes (utils.py:139-143): 15 layers, hidden 128, 512 codes, 10 modes (6,406,016 parameters), B=128,
    procedural weights: the first training forward's loss and logits digest, the digest of every parameter's gradient of
    that step (before clip_grad_norm_; the last layer's gate_v.bn gets none), two train_pixelcnn.py steps' losses."""
    import models
    _set_cpixelcnn_cfg(128, 15, 512, 10)
    torch.manual_seed(0)
    model = models.cpixelcnn(); model.train(True)
    assert sum(p.numel() for p in model.parameters()) == 6406016
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    seed = 4243
    model.load_state_dict(gu.procedural_state_generic(shapes, seed=seed))
    arrays = {'layout': _cgan_layout(shapes), 'sd_seed': np.array(seed)}
    g = torch.Generator().manual_seed(44)
    B = 128
    codes = torch.randint(0, 512, (B, 8, 8), generator=g)
    lab = torch.randint(0, 9, (B,), generator=g)              # mode 9 absent
    arrays['codes'] = codes.numpy(); arrays['label'] = lab.numpy()
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)
    losses = []
    for step in range(2):
        opt.zero_grad()
        out = model({'img': codes.clone(), 'label': lab})
        out['loss'].backward()
        if step == 0:
            arrays['logits0_digest'] = gu.checksum(out['logits'].detach())
            names, dead = [], []
            for k, p in model.named_parameters():
                if p.grad is None:
                    dead.append(k)
                    continue
                names.append(k)
                arrays['grad0_digest/' + k] = gu.checksum(p.grad)
                arrays['grad0_absmax/' + k] = np.array(float(p.grad.abs().max()))
            arrays['grad_keys'] = np.array(names)
            arrays['nograd_keys'] = np.array(dead)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1)
        opt.step()
        losses.append(out['loss'].item())
    arrays['losses'] = np.array(losses, dtype=np.float64)
    save('cpixelcnn_full_digest.npz', **arrays)


FIXTURES.update(cpixelcnn_small=fx_cpixelcnn_small, cpixelcnn_omniglot_small=fx_cpixelcnn_omniglot_small,
                cpixelcnn_full=fx_cpixelcnn_full)


# ---- CVAE (models/cvae.py): the conditional VAE baseline, label embeddings at the encoder input and the latent ----------
def _set_cvae_cfg(hidden, latent, classes, channels=3, data_name='CIFAR10'):
    cfg['model_name'] = 'cvae'; cfg['data_name'] = data_name; cfg['device'] = 'cpu'; cfg['classes_size'] = classes
    cfg['data_shape'] = [channels, 32, 32]
    cfg['vae'] = {'hidden_size': list(hidden), 'latent_size': latent, 'num_res_block': 2, 'embedding_size': 32}


def _cvae_small(name, classes, channels, data_name, full_final):
    """Widths [8, 16, 32], latent 16, embedding 32, B=8 with repeated and absent labels, procedural weights over the
    reference's layout (stored), 3 train_vae.py steps with the recorded noise: the first forward's outputs, the losses, the
    state after training (differences from the initial state, or digests only) and an eval-mode generate."""
    import models
    _set_cvae_cfg([8, 16, 32], 16, classes, channels, data_name)
    torch.manual_seed(0)
    model = models.cvae()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    seed = 1357
    sd0 = gu.procedural_state_generic(shapes, seed=seed)
    model.load_state_dict(sd0)
    model.train(True)
    arrays = {'layout': _cgan_layout(shapes), 'sd_seed': np.array(seed)}
    img, lab = gu.synthetic_batch(8, classes, seed=53, shape=(channels, 32, 32))
    lab[1] = lab[0]; lab[5] = lab[0]                         # a label held by three samples; most modes are absent
    lab[2] = classes - 1; lab[3] = 0
    arrays['img'] = img.numpy(); arrays['label'] = lab.numpy()
    first = _single_opt_steps(model, {'img': img, 'label': lab}, 600, 3, arrays)
    arrays['mu0'] = first['mu'].detach().numpy(); arrays['logvar0'] = first['logvar'].detach().numpy()
    arrays['img0'] = first['img'].detach().numpy()
    for k, v in model.state_dict().items():
        if not v.is_floating_point():
            arrays['sd_final_int/' + k] = v.numpy().copy()
        elif full_final:
            arrays['sd_delta/' + k] = (v - sd0[k]).detach().numpy()
        else:
            arrays['digest/' + k] = gu.checksum(v)
    model.train(False)
    z = torch.randn(8, 16, generator=torch.Generator().manual_seed(7))
    arrays['gen_z'] = z.numpy()
    with torch.no_grad():
        arrays['generated_eval'] = model.generate(lab, z).numpy()
    save(name, **arrays)


def fx_cvae_small():
    _cvae_small('cvae_small.npz', 10, 3, 'CIFAR10', True)


def fx_cvae_omniglot_small():
    _cvae_small('cvae_omniglot_small.npz', 1623, 1, 'Omniglot', False)


def fx_cvae_full():
    """Config widths (hidden [64, 128, 256], latent 128, embedding 32; 7,793,411 parameters with 10 modes), B=128,
    procedural weights: the first training forward's loss and mu / img digests, the digest of every parameter's gradient of
    that step (before clip_grad_norm_), two train_vae.py steps' losses, the recorded noise."""
    import models
    _set_cvae_cfg([64, 128, 256], 128, 10)
    torch.manual_seed(0)
    model = models.cvae(); model.train(True)
    assert sum(p.numel() for p in model.parameters()) == 7793411
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    seed = 9753
    model.load_state_dict(gu.procedural_state_generic(shapes, seed=seed))
    arrays = {'layout': _cgan_layout(shapes), 'sd_seed': np.array(seed)}
    B = 128
    img, _ = gu.synthetic_batch(B, 10, seed=3)
    lab = torch.randint(0, 9, (B,), generator=torch.Generator().manual_seed(46))          # mode 9 absent
    arrays['label'] = lab.numpy(); arrays['img_seed'] = np.array(3)
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)
    losses = []
    for step in range(2):
        with _PatchedNoise(700 + step) as pn:
            opt.zero_grad()
            out = model({'img': img.clone(), 'label': lab})
            out['loss'].backward()
        arrays[f'noise/{step}/0'] = pn.drawn[0].numpy()
        if step == 0:
            arrays['mu0_digest'] = gu.checksum(out['mu']); arrays['img0_digest'] = gu.checksum(out['img'])
            arrays['img0_sample'] = out['img'].detach().numpy()[:4, :, ::4, ::4].copy()
            names = []
            for k, p in model.named_parameters():
                names.append(k)
                arrays['grad0_digest/' + k] = gu.checksum(p.grad)
                arrays['grad0_absmax/' + k] = np.array(float(p.grad.abs().max()))
            arrays['grad_keys'] = np.array(names)
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1)
        opt.step()
        losses.append(out['loss'].item())
    arrays['losses'] = np.array(losses, dtype=np.float64)
    save('cvae_full_digest.npz', **arrays)


FIXTURES.update(cvae_small=fx_cvae_small, cvae_omniglot_small=fx_cvae_omniglot_small, cvae_full=fx_cvae_full)


# ---- CGlow (models/cglow.py): the conditional Glow baseline, a label-conditioned prior in the last block ------------------
def _cglow_small(name, channels, classes, steps, step_file=None):
    """CGlow [channels,32,32], K=2, L=3, hidden 32, B=4 with a repeated label, the last mode and most modes absent.  The
    zero-initialised ZeroConv2d weights, biases and scales (coupling nets, priors, embeddings) are perturbed from a seeded
    generator first -- at the all-zero initialisation the scale gradients vanish identically -- and the perturbed state is
    stored.  Then: ActNorm data init (first forward), `steps` train_glow.py steps with the gradients of the first one (before
    clip_grad_norm_), eval loss, reverse(reconstruct) and sampling from fixed z.  Later states are stored as the tensors
    that changed: sd_init/ whole, sd_final_delta/ as differences from the initialised state.  `step_file` takes the first
    step's gradients and the final differences where one file would be too large."""
    import models
    cfg['model_name'] = 'cglow'; cfg['device'] = 'cpu'; cfg['classes_size'] = classes
    cfg['data_shape'] = [channels, 32, 32]
    cfg['glow'] = {'hidden_size': 32, 'K': 2, 'L': 3, 'affine': True, 'conv_lu': True}
    torch.manual_seed(0); np.random.seed(0)
    model = models.cglow(); model.train(True)
    g = torch.Generator().manual_seed(97)
    with torch.no_grad():
        for mod in model.modules():
            if mod.__class__.__name__ == 'ZeroConv2d':
                for t in (mod.conv.weight, mod.conv.bias, mod.scale):
                    t.add_(0.02 * torch.randn(t.shape, generator=g))
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    arrays = np_state(sd0, 'sd/')
    arrays['layout'] = _cgan_layout({k: tuple(v.shape) for k, v in sd0.items()})
    img, lab = gu.synthetic_batch(4, classes, seed=57, shape=(channels, 32, 32))
    lab[0] = 1; lab[1] = classes - 1; lab[2] = 1; lab[3] = 0
    arrays['img'] = img.numpy(); arrays['label'] = lab.numpy()
    with _PatchedNoise(400) as pn, torch.no_grad():                       # train_glow.py:60-67 data-dependent init
        model({'img': img.clone(), 'label': lab})
    arrays['noise/init/0'] = pn.drawn[0].numpy()
    sdi = {k: v.detach().clone() for k, v in model.state_dict().items()}
    arrays.update(np_state({k: v for k, v in sdi.items() if not torch.equal(v, sd0[k])}, 'sd_init/'))
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)
    losses = []
    for s in range(steps):
        with _PatchedNoise(500 + s) as pn:
            opt.zero_grad()
            out = model({'img': img.clone(), 'label': lab})
            out['loss'].backward()
        arrays[f'noise/{s}/0'] = pn.drawn[0].numpy()
        if s == 0:
            for i, z in enumerate(out['z']):
                arrays[f'z0/{i}'] = z.detach().numpy()
            for k, p in model.named_parameters():
                if p.grad is not None:                                    # the split blocks' embeddings get none
                    arrays['grad0/' + k] = p.grad.detach().numpy().copy()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1)
        opt.step()
        losses.append(out['loss'].item())
    arrays['losses'] = np.array(losses, dtype=np.float64)
    for k, v in model.state_dict().items():
        if not torch.equal(v, sdi[k]):
            arrays['sd_final_delta/' + k] = (v - sdi[k]).detach().numpy()
    model.train(False)
    with torch.no_grad(), _PatchedNoise(600) as pn:
        out = model({'img': img.clone(), 'label': lab})
        arrays['noise/eval/0'] = pn.drawn[0].numpy()
        arrays['loss_eval'] = np.array(out['loss'].item())
        rec = model.reverse({'z': out['z'], 'label': lab, 'reconstruct': True})['img']
        arrays['reconstructed'] = rec.numpy()
        gz = [torch.randn(4, *s, generator=torch.Generator().manual_seed(7 + i)) * 0.7 for i, s in enumerate(model.make_z_shapes())]
        for i, z in enumerate(gz):
            arrays[f'gen_z/{i}'] = z.numpy()
        arrays['generated'] = model.generate(lab, gz).numpy()
    if step_file:                       # the 3-channel model's arrays do not fit one file of the size a committed file may have
        step = {k: arrays.pop(k) for k in list(arrays) if k.startswith(('grad0/', 'sd_final_delta/'))}
        save(step_file, **step)
    save(name, **arrays)


def fx_cglow_small():
    _cglow_small('cglow_small.npz', 1, 12, 2)


def fx_cglow_cifar_small():
    _cglow_small('cglow_cifar_small.npz', 3, 10, 2, step_file='cglow_cifar_small_step.npz')


def fx_cglow_omniglot_small():
    _cglow_small('cglow_omniglot_small.npz', 1, 1623, 1)


FIXTURES.update(cglow_small=fx_cglow_small, cglow_cifar_small=fx_cglow_cifar_small, cglow_omniglot_small=fx_cglow_omniglot_small)

# ---- MCGlow with additive coupling and / or the plain InvConv2d (cfg glow.affine / glow.conv_lu = False) ------------------------
def _mcglow_variant_small(name, channels, classes, affine, conv_lu, step_file=None):
    """MCGlow [channels,32,32], K=2, L=3, hidden 32, B=4 with a repeated label, built like _cglow_small: the zero-initialised
    ZeroConv2d tensors are perturbed from a seeded generator (at the all-zero initialisation the coupling networks' gradients
    vanish identically) and, for the plain InvConv2d, so is the orthogonal initial weight (at an orthogonal W, W^-T = W and
    the test of the log-determinant's gradient would be weak).  Contents as in fx_mcglow_small / _cglow_small: initial state,
    state after the ActNorm data init, batch, per-step noise, two train_glow.py steps' losses, grad0/* (before
    clip_grad_norm_), final state (as differences), loss_eval, z0/*, reconstructed, gen_z/*, generated.  `step_file` takes the
    first step's gradients and the final differences, as in _cglow_small."""
    import models
    cfg['model_name'] = 'mcglow'; cfg['device'] = 'cpu'; cfg['classes_size'] = classes; cfg['controller_rate'] = 0.5
    cfg['data_shape'] = [channels, 32, 32]
    cfg['glow'] = {'hidden_size': 32, 'K': 2, 'L': 3, 'affine': affine, 'conv_lu': conv_lu}
    torch.manual_seed(0); np.random.seed(0)
    model = models.mcglow(); model.train(True)
    g = torch.Generator().manual_seed(97)
    with torch.no_grad():
        for mod in model.modules():
            if mod.__class__.__name__ == 'ZeroConv2d':
                for t in (mod.conv.weight, mod.conv.bias, mod.scale):
                    t.add_(0.02 * torch.randn(t.shape, generator=g))
            if mod.__class__.__name__ == 'InvConv2d':
                c = mod.weight.shape[0]
                scale = 0.5 + 1.5 * torch.rand(c, generator=g)                 # singular values in [0.5, 2]
                mod.weight.copy_((mod.weight[:, :, 0, 0] * scale + 0.05 * torch.randn(c, c, generator=g))[:, :, None, None])
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    arrays = np_state(sd0, 'sd/')
    arrays['layout'] = _cgan_layout({k: tuple(v.shape) for k, v in sd0.items()})
    img, lab = gu.synthetic_batch(4, classes, seed=61, shape=(channels, 32, 32))
    lab[0] = 1; lab[1] = classes - 1; lab[2] = 1; lab[3] = 0
    arrays['img'] = img.numpy(); arrays['label'] = lab.numpy()
    with _PatchedNoise(400) as pn, torch.no_grad():                       # train_glow.py:60-67 data-dependent init
        model({'img': img.clone(), 'label': lab})
    arrays['noise/init/0'] = pn.drawn[0].numpy()
    sdi = {k: v.detach().clone() for k, v in model.state_dict().items()}
    arrays.update(np_state({k: v for k, v in sdi.items() if not torch.equal(v, sd0[k])}, 'sd_init/'))
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)
    losses = []
    for s in range(2):
        with _PatchedNoise(500 + s) as pn:
            opt.zero_grad()
            out = model({'img': img.clone(), 'label': lab})
            out['loss'].backward()
        arrays[f'noise/{s}/0'] = pn.drawn[0].numpy()
        if s == 0:
            for i, z in enumerate(out['z']):
                arrays[f'z0/{i}'] = z.detach().numpy()
            for k, p in model.named_parameters():
                arrays['grad0/' + k] = p.grad.detach().numpy().copy()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1)
        opt.step()
        losses.append(out['loss'].item())
    arrays['losses'] = np.array(losses, dtype=np.float64)
    for k, v in model.state_dict().items():
        if not torch.equal(v, sdi[k]):
            arrays['sd_final_delta/' + k] = (v - sdi[k]).detach().numpy()
    model.train(False)
    with torch.no_grad(), _PatchedNoise(600) as pn:
        out = model({'img': img.clone(), 'label': lab})
        arrays['noise/eval/0'] = pn.drawn[0].numpy()
        arrays['loss_eval'] = np.array(out['loss'].item())
        rec = model.reverse({'z': out['z'], 'label': lab, 'reconstruct': True})['img']
        arrays['reconstructed'] = rec.numpy()
        gz = [torch.randn(4, *s, generator=torch.Generator().manual_seed(7 + i)) * 0.7 for i, s in enumerate(model.make_z_shapes())]
        for i, z in enumerate(gz):
            arrays[f'gen_z/{i}'] = z.numpy()
        arrays['generated'] = model.generate(lab, gz).numpy()
    for k, v in arrays.items():                       # loss_fn zeroes NaN samples: a NaN in a fixture would hide errors
        assert v.dtype.kind != 'f' or np.isfinite(v).all(), k
    if step_file:                       # the 3-channel model's arrays do not fit one file of the size a committed file may have
        step = {k: arrays.pop(k) for k in list(arrays) if k.startswith(('grad0/', 'sd_final_delta/'))}
        save(step_file, **step)
    save(name, **arrays)


def fx_mcglow_additive_small():
    _mcglow_variant_small('mcglow_additive_small.npz', 1, 12, False, True)


def fx_mcglow_plainconv_small():
    _mcglow_variant_small('mcglow_plainconv_small.npz', 1, 12, True, False)


def fx_mcglow_plain_additive_cifar_small():
    _mcglow_variant_small('mcglow_plain_additive_cifar_small.npz', 3, 10, False, False,
                          step_file='mcglow_plain_additive_cifar_small_step.npz')


FIXTURES.update(mcglow_additive_small=fx_mcglow_additive_small, mcglow_plainconv_small=fx_mcglow_plainconv_small,
                mcglow_plain_additive_cifar_small=fx_mcglow_plain_additive_cifar_small)

# ---- create / transit on the label-embedding baselines (models/utils.py:47-88, 112-152) and the created set's DBI -------------
def _surgery_generate(model, name, label, x):
    """Eval-mode generate of the reference; cpixelcnn: the greedy decode (argmax per position through reference forwards,
    cpixelcnn.py:100-108 with the draw replaced) and the eval logits of the decoded map."""
    with torch.no_grad():
        if name != 'cpixelcnn':
            return {'gen': model.generate(label, x).numpy()}
        m = torch.zeros((label.numel(), 8, 8), dtype=torch.long)
        for i in range(8):
            for j in range(8):
                m[:, i, j] = model({'img': m, 'label': label})['logits'][:, :, i, j].argmax(1)
        return {'greedy': m.numpy(), 'logits': model({'img': m, 'label': label})['logits'].numpy()}


def _fx_surgery(name):
    """The reference's create (10 -> 14 modes, CPU, fixed seed) and transit(root 2, alpha in {0, 0.5, 1}) on the trained state of
    the model's *_small fixture (tests/surgery_util.base_state): only the tensors each call changes or adds, the state dict's
    key list after it, the inputs (C, x) and the eval-mode generate outputs.  The reference has no PixelCNN transit."""
    import models
    import surgery_util as su
    base = su.base_state(name)

    def fresh():
        su.configure(name, 'cpu', cfg)
        np.random.seed(0)
        m = getattr(models, name)()
        m.load_state_dict(base)
        m.train(False)
        return m

    arrays = {'create_seed': np.array(su.CREATE_SEED), 'root': np.array(su.ROOT), 'alphas': np.array(su.ALPHAS)}
    model = fresh()
    cfg['classes_size'] = su.NEW_MODES
    torch.manual_seed(su.CREATE_SEED)
    with torch.no_grad():                                                 # create.py:56 / transit.py:50 call both under no_grad
        models.utils.create(model)
    sd = model.state_dict()
    arrays['create_keys'] = np.array(list(sd))
    arrays.update(np_state(su.changed(sd, base), 'create/'))
    label, x = su.inputs(name, su.NEW_MODES)
    arrays.update({'create_out/' + k: v for k, v in _surgery_generate(model, name, label, x).items()})
    cfg['classes_size'] = su.MODES
    if name != 'cpixelcnn':
        model = fresh()
        label, x = su.inputs(name, su.MODES)
        for i, alpha in enumerate(su.ALPHAS):
            with torch.no_grad():
                models.utils.transit(model, su.ROOT, alpha)
            sd = model.state_dict()
            arrays['transit_keys'] = np.array(list(sd))
            arrays.update(np_state(su.changed(sd, base), f'transit{i}/'))
            arrays.update({f'transit{i}_out/' + k: v for k, v in _surgery_generate(model, name, label, x).items()})
    save(f'surgery_{name}.npz', **arrays)


def fx_surgery_cgan():
    _fx_surgery('cgan')


def fx_surgery_cvae():
    _fx_surgery('cvae')


def fx_surgery_cglow():
    _fx_surgery('cglow')


def fx_surgery_cpixelcnn():
    _fx_surgery('cpixelcnn')


def fx_dbi():
    """scikit-learn's davies_bouldin_score on the three cases of tests/dbi_ref.py (inputs regenerated from their seeds): on the
    float64 copy, and on the float32 rows themselves -- what the reference's DBI (metrics.py:164-166) computes."""
    from sklearn.metrics import davies_bouldin_score
    import dbi_ref
    arrays = {'cases': np.array(list(dbi_ref.CASES))}
    for name, (n, d, seed) in dbi_ref.CASES.items():
        x, label = dbi_ref.make_case(name)
        arrays[name + '/shape_seed'] = np.array([n, d, seed])
        arrays[name + '/checksum'] = np.array([float(x.astype(np.float64).sum()), float(label.sum())])
        arrays[name + '/sklearn_f64'] = np.array(davies_bouldin_score(x.astype(np.float64), label))
        arrays[name + '/sklearn_f32'] = np.array(davies_bouldin_score(x, label), dtype=np.float64)
    save('dbi.npz', **arrays)


FIXTURES.update(surgery_cgan=fx_surgery_cgan, surgery_cvae=fx_surgery_cvae, surgery_cglow=fx_surgery_cglow,
                surgery_cpixelcnn=fx_surgery_cpixelcnn, dbi=fx_dbi)


# ---- short batches: the first n samples of a small fixture's batch, the reference in float64 and in float32 -----------------
class _GivenNoise:
    """torch.rand_like / torch.randn_like return `noise` (cast to the asking tensor's dtype): the fixture's recorded draw."""

    def __init__(self, noise):
        self.noise = noise

    def __enter__(self):
        self._randn_like, self._rand_like = torch.randn_like, torch.rand_like
        torch.randn_like = torch.rand_like = lambda t, **k: self.noise.to(t.dtype)
        return self

    def __exit__(self, *a):
        torch.randn_like, torch.rand_like = self._randn_like, self._rand_like


class _FloatFollows:
    """The reference writes `.float()` on its one-hot indicators; while a float64 model runs, `.float()` gives `dtype`."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self._float = torch.Tensor.float
        torch.Tensor.float = lambda t, *a, **k: t.to(self.dtype)
        return self

    def __exit__(self, *a):
        torch.Tensor.float = self._float


def _short_record(arrays, n, full, run):
    """`run(dtype) -> (loss, {name: gradient}, extras)` of one training-mode forward + backward of the reference on the
    first n samples.  Stored under n<n>/: the float64 loss and the float32 one, the float64 gradients -- whole when `full`,
    else per parameter their norm, sum and max |g| (the digest form of vqvae_train_full_digest.npz) -- the same from the
    float32 run, and per parameter max |g32 - g64|: the reference's own rounding, which the short-batch bounds rest on."""
    l64, g64, extra = run(torch.float64)
    l32, g32, _ = run(torch.float32)
    assert l64.dtype == torch.float64 and l32.dtype == torch.float32 and set(g64) == set(g32)
    names = sorted(g64)
    p = f'n{n}/'
    arrays[p + 'loss'] = np.array(l64.item()); arrays[p + 'loss_fp32'] = np.array(l32.item(), dtype=np.float32)
    arrays[p + 'grad_names'] = np.array(names)
    for tag, g in (('', g64), ('_fp32', g32)):
        assert all(g[k].dtype == (torch.float32 if tag else torch.float64) for k in names)
        if full:
            for k in names:
                arrays[p + f'grad{tag}/' + k] = g[k].numpy().copy()
        else:
            arrays[p + 'grad_norms' + tag] = np.array([g[k].double().norm().item() for k in names])
            arrays[p + 'grad_sums' + tag] = np.array([g[k].double().sum().item() for k in names])
            arrays[p + 'grad_maxabs' + tag] = np.array([g[k].double().abs().max().item() for k in names])
    arrays[p + 'grad_numel'] = np.array([g64[k].numel() for k in names], dtype=np.int64)
    arrays[p + 'fp32_err'] = np.array([(g32[k].double() - g64[k]).abs().max().item() for k in names])
    for k, v in extra.items():
        arrays[p + k] = v
    print(f'  n={n}: loss {l64.item():.9f}  fp32 off by {abs(l32.item() - l64.item()):.2e}  worst gradient fp32 error / max|g| '
          f'{max(float((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max().clamp_min(1e-30)) for k in names):.2e}')


def fx_vqvae_train_short():
    """The VQ-VAE training forward + backward (train_vqvae.py:103-105) from vqvae_train_small.npz's state on the first
    n = 1, 3 and 7 samples of its batch of 8: a loader's short final batch.  n = 3 whole, 1 and 7 as digests; with each the
    code map and the arg-min margin of the float64 run (the float32 run must pick the same codes)."""
    import models
    d = gu.load_npz('vqvae_train_small.npz')
    _set_vqvae_cfg([16, 16], 8, 64)
    img = torch.from_numpy(d['img'])
    arrays = {}
    for n in (1, 3, 7):
        codes = []

        def run(dtype):
            torch.manual_seed(0)
            model = models.vqvae()
            model.load_state_dict(gu.state_from_npz(d))
            model = model.to(dtype); model.train(True)
            seen = {}
            h = model.quantizer.register_forward_pre_hook(lambda mod, inp: seen.update(x=inp[0].detach().clone(), emb=mod.embedding.clone()))
            out = model({'img': img[:n].to(dtype).clone()})
            h.remove()
            out['loss'].backward()
            codes.append(out['code'].clone())
            extra = {'code': out['code'].numpy().copy(), 'dist_margin': _vq_margin(seen['x'], seen['emb']).numpy()}
            return out['loss'].detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}, extra
        _short_record(arrays, n, n == 3, run)
        assert torch.equal(codes[0], codes[1]), 'float32 and float64 disagree on a code: the error measured is no rounding error'
    save('vqvae_train_short.npz', **arrays)


def fx_cglow_short():
    """The CGlow training forward + backward (train_glow.py:110-112) from cglow_small.npz's initialised state (its sd/ with
    sd_init/ over it) on the first n = 1 and 3 samples of its batch of 4, with the first n rows of its recorded
    dequantisation noise (noise/0/0).  n = 3 (= B - 1) whole, n = 1 as a digest.  Parameters the reference gives no
    gradient (the split blocks' embeddings) are absent from grad_names, as in cglow_small.npz."""
    import models
    import cglow_ref
    d = gu.load_npz('cglow_small.npz')
    _, init, _ = cglow_ref.states(d)
    cfg['model_name'] = 'cglow'; cfg['device'] = 'cpu'; cfg['classes_size'] = 12
    cfg['data_shape'] = [1, 32, 32]
    cfg['glow'] = dict(cglow_ref.GLOW_CFG)
    img, lab, noise = torch.from_numpy(d['img']), torch.from_numpy(d['label']), torch.from_numpy(d['noise/0/0'])
    arrays = {}
    for n in (1, 3):
        def run(dtype):
            torch.manual_seed(0); np.random.seed(0)
            model = models.cglow()
            model.load_state_dict(init)
            model = model.to(dtype); model.train(True)
            with _GivenNoise(noise[:n]), _FloatFollows(dtype):
                out = model({'img': img[:n].to(dtype).clone(), 'label': lab[:n]})
                out['loss'].backward()
            grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
            return out['loss'].detach(), grads, {}
        _short_record(arrays, n, n == 3, run)
    save('cglow_short.npz', **arrays)


FIXTURES.update(vqvae_train_short=fx_vqvae_train_short, cglow_short=fx_cglow_short)

if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None)
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    for name, fn in FIXTURES.items():
        if a.only in (None, name):
            fn()
