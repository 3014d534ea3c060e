"""MCGlow at the CIFAR-10 shape ([3, 32, 32], 10 modes, hidden 32, L = 3, B = 4) on the HIP path against the fp64 CPU
oracle: 12 / 24 / 48 channels per level (6 / 12 / 24 after each split, 12 of them in a 16-wide NHWC row) and 48 x 48 LU
matrices, which the 1-channel tests of test_mcglow_gpu.py never build.  K = 9 gives 27 flows, so every batched
per-module launch (MCGEN_GLOW_BATCH_MAX jobs) splits in two.

The oracle runs in float64 on the fp32 weights the GPU model holds (the MultimodalController codebooks stay fp32; they
are 0/1 masks).  The bounds are those of the 1-channel model tests, which measure the same fp32 path: 1e-4 bits/dim on
the loss, 5e-4 of the tensor's max on the latents, 2e-3 of the max on the ActNorm init, 2e-4 max|g| + 1e-6 on every
gradient, 1e-3 of the max on images; bf16 compute is held to 2e-2 bits/dim."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES, K_SMALL = 10, 2
FIXED = ('w_p', 'u_mask', 'l_mask', 's_sign', 'l_eye', 'codebook')


def _rel(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _cfg(K):
    from mcgen_amd.config import cfg
    cfg.update(model_name='mcglow', device='cuda', classes_size=MODES, controller_rate=0.5, data_shape=[3, 32, 32],
               compute_dtype='float32')
    cfg['glow'] = {'hidden_size': 32, 'K': K, 'L': 3, 'affine': True, 'conv_lu': True}


def _fresh_state(K):
    """The model's own initial weights (NumPy-seeded LU factors, ActNorms not yet initialised), on the CPU."""
    from mcgen_amd import models
    _cfg(K)
    np.random.seed(0)
    torch.manual_seed(0)
    return {k: v.clone() for k, v in models.mcglow().state_dict().items()}


def _model(K, sd):
    from mcgen_amd import models
    _cfg(K)
    np.random.seed(0)
    m = models.mcglow()
    m.load_state_dict(sd)
    return m.cuda()


def _to64(sd):
    return {k: (v.double() if v.dtype.is_floating_point and not k.endswith('codebook') else v.clone()) for k, v in sd.items()}


def _to32(sd):
    return {k: (v.float() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}


def _data(seed=21):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (4, 3, 32, 32), generator=g).float() / 255 * 2 - 1
    lab = torch.randint(0, MODES, (4,), generator=g)
    return img, lab, torch.rand(img.shape, generator=g), torch.rand(img.shape, generator=g)


def _initialised_state(K, img, lab, noise_init):
    """The fp64 oracle's data-dependent ActNorm init from the model's fresh weights, as fp32, with the zero-initialised
    ZeroConv2d weights and scales perturbed (as test_mcglow_gradients_vs_oracle does) so every path carries gradient."""
    from oracle import mcglow_oracle as G
    sd64 = _to64(_fresh_state(K))
    with torch.no_grad():
        G.forward(sd64, img.double(), lab, MODES, K, 3, noise_init.double(), train=True)
    init = _to32(sd64)
    g = torch.Generator().manual_seed(11)
    for k in init:
        if '.conv.weight' in k or k.endswith('prior.scale') or k.endswith('8.module.scale'):
            init[k] = init[k] + 0.02 * torch.randn(init[k].shape, generator=g)
    return sd64, init


def _oracle_grads(sd, K, img, lab, noise):
    from oracle import mcglow_oracle as G
    sdg = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point and not k.endswith(FIXED) else v.clone())
           for k, v in _to64(sd).items()}
    out = G.forward(sdg, img.double(), lab, MODES, K, 3, noise.double(), train=True)
    out['loss'].backward()
    return (float(out['loss'].detach()), [z.detach() for z in out['z']],
            {k: v.grad for k, v in sdg.items() if v.requires_grad and v.grad is not None})


@pytest.mark.parametrize('K', [2, 9])
def test_mcglow_cifar_init_loss_latents_gradients(K):
    """First training forward: ActNorm data init (loc / scale) against the oracle's init.  Then, on the oracle's
    initialised weights (perturbed), the training loss, every latent z and every parameter gradient."""
    img, lab, noise_init, noise = _data()
    sd64, init = _initialised_state(K, img, lab, noise_init)
    m = _model(K, _fresh_state(K))
    m.train(True)
    with torch.no_grad():
        m({'img': img.cuda(), 'label': lab.cuda(), 'noise': noise_init.cuda()})
    got = m.state_dict()
    n_an = 0
    for k, v in sd64.items():
        if k.endswith(('actnorm.loc', 'actnorm.scale', '1.module.loc', '1.module.scale', '5.module.loc', '5.module.scale')):
            assert float((got[k].double().cpu() - v).abs().max()) < 2e-3 * float(v.abs().max()) + 1e-5, k
            n_an += 1
        if k.endswith('initialized'):
            assert int(got[k]) == 1, k
    assert n_an == 2 * 3 * K * 3                      # loc + scale of 3 ActNorms per flow, 3K flows
    loss_ref, z_ref, gref = _oracle_grads(init, K, img, lab, noise)
    m = _model(K, init)
    m.train(True)
    out = m({'img': img.cuda(), 'label': lab.cuda(), 'noise': noise.cuda()})
    loss = float(out['loss'].detach())
    assert abs(loss - loss_ref) < 1e-4, (loss, loss_ref)
    assert [tuple(z.shape) for z in out['z']] == [tuple(z.shape) for z in z_ref] == [(4, 6, 16, 16), (4, 12, 8, 8), (4, 48, 4, 4)]
    for i, (z, zr) in enumerate(zip(out['z'], z_ref)):
        assert _rel(z, zr) < 5e-4, i
    out['loss'].backward()
    named = dict(m.named_parameters())
    assert set(gref) == set(named), set(gref) ^ set(named)
    worst = 0.0
    for k, gr in gref.items():
        gg = named[k].grad
        assert gg is not None, k
        err = float((gg.double().cpu() - gr).abs().max())
        tol = 2e-4 * float(gr.abs().max()) + 1e-6
        assert err < tol, (k, err, tol)
        worst = max(worst, err / tol)
    print(f'K={K}: loss {loss} vs {loss_ref}; worst gradient err/tol {worst:.3f}')


def test_mcglow_cifar_reverse_and_generate():
    """reverse(reconstruct=True) of the eval-mode latents gives back the dequantised input image, and generate() equals
    the fp64 oracle.reverse on the same z and labels."""
    from oracle import mcglow_oracle as G
    img, lab, noise_init, noise = _data()
    _, init = _initialised_state(K_SMALL, img, lab, noise_init)
    m = _model(K_SMALL, init)
    m.train(False)
    with torch.no_grad():
        out = m({'img': img.cuda(), 'label': lab.cuda(), 'noise': noise.cuda()})
        rec = m.reverse({'z': out['z'], 'label': lab.cuda(), 'reconstruct': True})['img']
        assert _rel(rec, torch.clamp(img * 0.5 + noise / 256, -.5, .5) * 2) < 1e-3
        g = torch.Generator().manual_seed(5)
        gz = [torch.randn(4, *s, generator=g) for s in m.make_z_shapes()]
        gen = m.generate(lab.cuda(), [z.cuda() for z in gz])
    ref = G.reverse(_to64(init), [z.double() for z in gz], lab, MODES, K_SMALL, 3, reconstruct=False)
    assert gen.shape == (4, 3, 32, 32)
    assert _rel(gen, ref) < 1e-3


def test_mcglow_cifar_bf16_tracks_fp64():
    """bf16 compute (fp32 accumulation and log-determinants) at the CIFAR-10 shape: the training-mode loss is within
    2e-2 bits/dim of the fp64 oracle."""
    from oracle import mcglow_oracle as G
    img, lab, noise_init, noise = _data()
    _, init = _initialised_state(K_SMALL, img, lab, noise_init)
    with torch.no_grad():
        ref = float(G.forward(_to64(init), img.double(), lab, MODES, K_SMALL, 3, noise.double(), train=True)['loss'])
        m = _model(K_SMALL, init).set_compute_dtype(torch.bfloat16)
        m.train(True)
        got = float(m({'img': img.cuda(), 'label': lab.cuda(), 'noise': noise.cuda()})['loss'])
    assert abs(got - ref) < 2e-2, (got, ref)


def _run(init, img, lab, noise, gz):
    m = _model(K_SMALL, init)
    m.train(True)
    out = m({'img': img.cuda(), 'label': lab.cuda(), 'noise': noise.cuda()})
    out['loss'].backward()
    res = {'loss': out['loss'].detach().clone()}
    res.update({f'z{i}': z.detach().clone() for i, z in enumerate(out['z'])})
    res.update({'grad/' + k: p.grad.detach().clone() for k, p in m.named_parameters()})
    m.train(False)
    with torch.no_grad():
        res['generated'] = m.generate(lab.cuda(), [z.cuda() for z in gz]).clone()
    torch.cuda.synchronize()
    return res


def _poison_allocator():
    """Fill the caching allocator's free blocks with NaN: 1 MiB tensors fill whole 2 MiB small-pool segments, 4 MiB
    ones split 20 MiB large-pool segments, 64 MiB ones take segments of their own."""
    held = [torch.empty(1 << 18, device='cuda') for _ in range(512)]
    held += [torch.empty(1 << 20, device='cuda') for _ in range(40)]
    held += [torch.empty(1 << 24, device='cuda') for _ in range(4)]
    for t in held:
        t.fill_(float('nan'))
    torch.cuda.synchronize()
    del held


def test_mcglow_cifar_padding_under_poisoned_allocator():
    """Padded NHWC channels never reach a result: with the allocator's free memory full of NaN (every torch.empty of the
    pass returns NaN-filled memory, glow_unsqueeze's output included), the loss, latents, gradients and generated images
    of a training step and a sampling pass are finite and bit-identical to a clean run.  The Glow path's reductions run in
    a fixed order, so the two runs must agree exactly."""
    img, lab, noise_init, noise = _data()
    _, init = _initialised_state(K_SMALL, img, lab, noise_init)
    g = torch.Generator().manual_seed(6)
    _cfg(K_SMALL)
    gz = [torch.randn(4, 6, 16, 16, generator=g), torch.randn(4, 12, 8, 8, generator=g), torch.randn(4, 48, 4, 4, generator=g)]
    clean = _run(init, img, lab, noise, gz)
    torch.cuda.empty_cache()
    _poison_allocator()
    poisoned = _run(init, img, lab, noise, gz)
    assert set(clean) == set(poisoned)
    for k, v in clean.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(poisoned[k], v), (k, float((poisoned[k] - v).abs().max()))
