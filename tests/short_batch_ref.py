"""References of the short-batch tests (test_short_batch_gpu.py, test_short_batch_ref_cpu.py): for each of the eight
single-network models, its small fixture's configuration, state and batch of B samples, and the loss and every parameter's
gradient of ONE training-mode forward + backward on the first n samples of that batch (labels and recorded noise sliced
alike) -- a loader's short final batch.

Six models have a callable restatement, which runs here on the CPU in the dtype asked for (float64 is the reference, float32
measures the reference's own rounding): the oracles of MCVAE, MCGlow, MCPixelCNN and the classifier (+ F.cross_entropy),
cvae_ref.py and cpixelcnn_ref.py.  The VQ-VAE training step and CGlow have none: tools/gen_golden.py ran the reference
itself at those n in both dtypes and stored the results (vqvae_train_short.npz, cglow_short.npz: n = 3 whole, the other
sizes as per-parameter norm / sum / max |g|).

Bounds.  Each model starts from the bound its own gradient-vs-reference test uses at batch B (quoted in SPECS with the
test it comes from).  A small N thins the BatchNorm statistics, so the bound of a (model, n) is the larger of that and
4 x the float32-vs-float64 error of the reference alone (`bounds`); 4, because the kernels reorder sums that the float32
restatement does in torch's order.  test_short_batch_ref_cpu.py prints those errors and asserts each within a quarter of
its bound."""
from __future__ import annotations

import functools
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

import cglow_ref
import golden_util as gu


class Spec(NamedTuple):
    B: int                      # the fixture's batch size
    loss_abs: float             # |loss - ref| bound ...
    loss_rel: float             # ... + this x |ref|
    grad_rel: float             # per parameter: max |g - ref| < grad_rel x max |ref| + grad_abs
    grad_abs: float
    bf16_loss: float            # |bf16 loss - fp32 loss| (x |loss| for the classifier): the model's "bf16 tracks fp32" bound
    one_ok: bool                # a training step on one sample is legal


# quoted from: test_mcvae_gpu.py::test_mcvae_gradients_vs_oracle / test_mcvae_bf16_tracks_fp32;
# test_cvae_gpu.py::test_gradients_vs_fp64_restatement / test_graphed_step_equals_eager_and_bf16_tracks_fp32;
# test_mcglow_gpu.py::test_mcglow_gradients_vs_oracle / test_mcglow_bf16_tracks_fp32;
# test_cglow_gpu.py::test_cglow_forward_init_and_reverse (loss) / test_cglow_gradients_vs_reference / test_cglow_bf16_tracks_fp32;
# test_mcpixelcnn_gpu.py::test_pixelcnn_gradients_vs_oracle / test_pixelcnn_bf16_tracks_fp32;
# test_cpixelcnn_gpu.py::test_cpixelcnn_vs_reference (loss) / test_gradients_vs_reference_autograd / test_graphed_step_..._bf16_...;
# test_vqvae_train_gpu.py::test_vqvae_small_step0_and_steps_match_reference / test_vqvae_bf16_tracks_fp32_fixture;
# test_classifier_train_gpu.py::test_classifier_train_small_matches_reference (2e-5 relative on the loss and on every
# gradient, conv biases in front of a BatchNorm < 1e-5 absolute; bf16 loss 1e-2 relative)
SPECS: Dict[str, Spec] = {
    'mcvae': Spec(8, 1e-5, 0.0, 5e-4, 2e-7, 1e-2, False),
    'cvae': Spec(8, 1e-5, 0.0, 5e-4, 1e-7, 1e-2, False),
    'mcglow': Spec(4, 1e-4, 0.0, 2e-4, 1e-6, 2e-2, True),
    'cglow': Spec(4, 1e-4, 0.0, 2e-4, 1e-6, 2e-2, True),
    'mcpixelcnn': Spec(6, 1e-4, 0.0, 5e-4, 2e-6, 2e-2, True),
    'cpixelcnn': Spec(6, 1e-4, 0.0, 5e-4, 1e-7, 5e-2, True),
    'vqvae': Spec(8, 1e-5, 0.0, 5e-4, 2e-7, 1e-2, True),
    'classifier': Spec(16, 0.0, 2e-5, 2e-5, 0.0, 1e-2, True),
}
MODELS = list(SPECS)
CLASSIFIER = ([3, 32, 32], 100, 7411)                       # test_classifier_train_gpu.py SMALL['coil100']
CLASSIFIER_CONV_BIASES = ('blocks.0.bias', 'blocks.4.bias', 'blocks.8.bias', 'blocks.12.bias')
_NOGRAD = ('running_mean', 'running_var', 'num_batches_tracked', 'codebook', 'initialized', 'w_p', 'u_mask', 'l_mask', 's_sign',
           'l_eye')


def sizes(name):
    """The short sizes of a model: 1, 3 and B - 1 (3 = B - 1 for the Glows)."""
    return sorted({1, 3, SPECS[name].B - 1})


class Ref(NamedTuple):
    loss: float
    grads: Optional[Dict[str, Optional[torch.Tensor]]]   # whole gradients (None: the reference gives that parameter none)
    digest: Optional[Dict[str, tuple]]                   # or per parameter (norm, sum, max |g|, numel)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return cglow_ref.load({'mcvae': 'mcvae_small.npz', 'cvae': 'cvae_small.npz', 'mcglow': 'mcglow_small.npz', 'cglow': 'cglow_small.npz',
                           'mcpixelcnn': 'mcpixelcnn_small.npz', 'cpixelcnn': 'cpixelcnn_small.npz', 'vqvae': 'vqvae_train_small.npz',
                           'classifier': 'classifier_train_small.npz'}[name])


@functools.lru_cache(maxsize=None)
def _state(name):
    d = fixture(name)
    if name in ('mcvae', 'mcpixelcnn', 'vqvae'):
        return gu.state_from_npz(d)
    if name in ('cvae', 'cpixelcnn'):
        return gu.procedural_state_generic(cglow_ref.layout(d), seed=int(d['sd_seed']))
    if name == 'cglow':
        return cglow_ref.states(d)[1]
    if name == 'mcglow':                  # as test_mcglow_gradients_vs_oracle: the ZeroConv2d weights perturbed off zero
        init = gu.state_from_npz(d, 'sd_init/')
        g = torch.Generator().manual_seed(11)
        for k in init:
            if '.conv.weight' in k or k.endswith('prior.scale') or k.endswith('8.module.scale'):
                init[k] = init[k] + 0.02 * torch.randn(init[k].shape, generator=g)
        return init
    shapes = {k[len('coil100/sd_final/'):]: tuple(v.shape) for k, v in d.items() if k.startswith('coil100/sd_final/')}
    full = dict(shapes, **{'classifier.weight': (100, 1024)})          # (the fixture stores every 4th row of the final head)
    return gu.procedural_state_generic(full, seed=CLASSIFIER[2])


def state(name):
    """A fresh copy of the model's starting state (reference state_dict keys)."""
    return {k: v.clone() for k, v in _state(name).items()}


@functools.lru_cache(maxsize=None)
def _batch(name):
    d = fixture(name)
    if name in ('mcvae', 'cvae'):
        return {'img': torch.from_numpy(d['img']), 'label': torch.from_numpy(d['label']), 'eps': torch.from_numpy(d['noise/0/0'])}
    if name in ('mcglow', 'cglow'):
        return {'img': torch.from_numpy(d['img']), 'label': torch.from_numpy(d['label']), 'noise': torch.from_numpy(d['noise/0/0'])}
    if name in ('mcpixelcnn', 'cpixelcnn'):
        return {'img': torch.from_numpy(d['codes']), 'label': torch.from_numpy(d['label'])}
    if name == 'vqvae':
        return {'img': torch.from_numpy(d['img'])}
    img, lab = gu.synthetic_batch(16, CLASSIFIER[1], seed=int(d['coil100/input_seed']), shape=tuple(CLASSIFIER[0]))
    return {'img': img, 'label': lab}


def batch(name, n=None):
    """The model's input dict on the CPU: the first n samples of the fixture's batch (all B when n is None)."""
    return {k: v[:n].clone() for k, v in _batch(name).items()}


def _params(sd, dtype):
    """Floating tensors in `dtype`, the trainable ones as leaves that take a gradient; the rest cloned as they are."""
    out = {}
    for k, v in sd.items():
        if v.dtype.is_floating_point:
            v = v.to(dtype).clone()
            if not k.endswith(_NOGRAD):
                v.requires_grad_(True)
        else:
            v = v.clone()
        out[k] = v
    return out


def restate(name, n, dtype):
    """The callable restatement on the first n samples in `dtype` -> (loss tensor, {name: gradient or None})."""
    b = batch(name, n)
    fl = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in b.items()}
    if name == 'cpixelcnn':
        from cpixelcnn_ref import ref_module
        ref = ref_module(state(name), 10, dtype)
        loss = ref(fl['img'], fl['label'])
        loss.backward()
        return loss.detach(), {k: (None if p.grad is None else p.grad) for k, p in ref.named_parameters()}
    P = _params(state(name), dtype)
    if name == 'mcvae':
        from oracle import mcvae_oracle as O
        loss = O.forward(P, fl['img'], fl['label'], 10, [8, 16, 32], 2, train=True, eps=fl['eps'])['loss']
    elif name == 'cvae':
        from cvae_ref import ref_forward
        P = {k: v for k, v in P.items() if v.requires_grad}
        loss = ref_forward(P, fl['img'], fl['label'], fl['eps'])
    elif name == 'mcglow':
        from oracle import mcglow_oracle as O
        loss = O.forward(P, fl['img'], fl['label'], 12, 2, 3, fl['noise'], train=True)['loss']
    elif name == 'mcpixelcnn':
        from oracle import mcpixelcnn_oracle as O
        loss = O.forward(P, fl['img'], fl['label'], 10, train=True)['loss']
    elif name == 'classifier':
        from oracle import classifier_oracle as O
        x = O.encode(P, fl['img'], train=True)
        loss = F.cross_entropy(F.linear(x.reshape(x.shape[0], -1), P['classifier.weight'], P['classifier.bias']), fl['label'])
    else:
        raise KeyError(f'{name} has no callable restatement: its short batches are fixtures')
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in P.items() if v.requires_grad}


def _digest(g):
    g = g.double()
    return float(g.norm()), float(g.sum()), float(g.abs().max()), g.numel()


@functools.lru_cache(maxsize=None)
def _stored(name, n, tag):
    d = gu.load_npz({'vqvae': 'vqvae_train_short.npz', 'cglow': 'cglow_short.npz'}[name])
    p = f'n{n}/'
    names = [str(k) for k in d[p + 'grad_names']]
    loss = float(d[p + 'loss' + tag])
    if p + 'grad/' + names[0] in d:
        return Ref(loss, {k: torch.from_numpy(d[p + f'grad{tag}/' + k]) for k in names}, None), dict(zip(names, d[p + 'fp32_err']))
    dig = {k: (float(a), float(b), float(c), int(m)) for k, a, b, c, m in
           zip(names, d[p + 'grad_norms' + tag], d[p + 'grad_sums' + tag], d[p + 'grad_maxabs' + tag], d[p + 'grad_numel'])}
    return Ref(loss, None, dig), dict(zip(names, d[p + 'fp32_err']))


@functools.lru_cache(maxsize=None)
def reference(name, n, dtype=torch.float64) -> Ref:
    """The reference at (model, n), computed once and shared; callers leave it unchanged."""
    if name in ('vqvae', 'cglow'):
        return _stored(name, n, '' if dtype == torch.float64 else '_fp32')[0]
    loss, grads = restate(name, n, dtype)
    return Ref(float(loss), grads, None)


def _maxabs(ref: Ref, k):
    return ref.digest[k][2] if ref.grads is None else float(ref.grads[k].double().abs().max())


@functools.lru_cache(maxsize=None)
def fp32_error(name, n):
    """-> (|loss32 - loss64|, {parameter: max |g32 - g64|}): the error of the float32 reference against the float64 one."""
    r64, r32 = reference(name, n), reference(name, n, torch.float32)
    if name in ('vqvae', 'cglow'):
        return abs(r32.loss - r64.loss), dict(_stored(name, n, '')[1])
    return abs(r32.loss - r64.loss), {k: float((r32.grads[k].double() - g).abs().max()) for k, g in r64.grads.items() if g is not None}


def bounds(name, n):
    """-> (loss bound, {parameter: elementwise gradient bound}) of (model, n): see the module docstring."""
    s, ref = SPECS[name], reference(name, n)
    eloss, egrad = fp32_error(name, n)
    names = ref.digest if ref.grads is None else [k for k, g in ref.grads.items() if g is not None]
    out = {}
    for k in names:
        base = s.grad_rel * _maxabs(ref, k) + s.grad_abs
        if name == 'classifier' and k in CLASSIFIER_CONV_BIASES:
            base = 1e-5
        out[k] = max(base, 4 * egrad[k])
    return max(s.loss_abs + s.loss_rel * abs(ref.loss), 4 * eloss), out


def check_gradient(name, n, k, got: Optional[torch.Tensor]):
    """Compare one parameter's gradient from the GPU with the reference at (model, n) -> (error, bound) for the report;
    raises AssertionError outside the bound.  Whole gradients: max |g - ref| < bound.  Digests: an elementwise error below
    `bound` moves the norm by at most sqrt(numel) x bound and the sum by at most numel x bound, and max |g| by bound."""
    ref = reference(name, n)
    if ref.grads is not None and ref.grads.get(k) is None or ref.grads is None and k not in ref.digest:
        assert got is None or float(got.abs().max()) == 0.0, (name, n, k, 'the reference gives this parameter no gradient')
        return 0.0, 0.0
    assert got is not None, (name, n, k)
    bound = bounds(name, n)[1][k]
    g = got.detach().double().cpu()
    if ref.grads is not None:
        err = float((g - ref.grads[k].double()).abs().max())
        assert err < bound, (name, n, k, err, bound)
        return err, bound
    norm, total, mx, numel = ref.digest[k]
    assert g.numel() == numel, (name, n, k)
    e_norm, e_sum, e_max = abs(float(g.norm()) - norm), abs(float(g.sum()) - total), abs(float(g.abs().max()) - mx)
    assert e_norm < np.sqrt(numel) * bound and e_sum < numel * bound and e_max < bound, (name, n, k, e_norm, e_sum, e_max, bound)
    return e_max, bound
