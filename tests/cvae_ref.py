"""Torch restatement of the CVAE baseline's training-mode forward (reference: models/cvae.py), as a pure function over a dict
of parameters.  It follows the dtype it is given: the gradient tests run it in float64, the short-batch reference test
also in float32 to measure the reference's own rounding.  Shared by test_cvae_gpu.py and the short-batch tests."""
import torch
import torch.nn.functional as F


def ref_forward(P, img, lab, eps, nstage=3, nres=2):
    """CVAE's training-mode forward (cvae.py:131-142) over a dict of parameters -> loss, in the dtype of P / img / eps."""
    def bn(x, pre):
        return F.batch_norm(x, None, None, P[pre + '.weight'], P[pre + '.bias'], True, 0.1, 1e-5)

    def res(x, pre):
        h = torch.relu(bn(F.conv2d(x, P[pre + '.conv.0.weight'], P[pre + '.conv.0.bias'], padding=1), pre + '.conv.1'))
        h = bn(F.conv2d(h, P[pre + '.conv.3.weight'], P[pre + '.conv.3.bias'], padding=1), pre + '.conv.4')
        return torch.relu(h + x)
    x01 = (img + 1) / 2
    n = img.shape[0]
    e = P['encoder.embedding.weight'].t()[lab]
    x = torch.cat([x01, e[:, :, None, None].expand(n, e.shape[1], *img.shape[2:])], 1)
    for i in range(nstage):
        q = f'encoder.blocks.{3 * i}'
        x = torch.relu(bn(F.conv2d(x, P[q + '.weight'], P[q + '.bias'], stride=2, padding=1), f'encoder.blocks.{3 * i + 1}'))
    for r in range(nres):
        x = res(x, f'encoder.blocks.{3 * nstage + r}')
    shape = x.shape[1:]
    x = x.reshape(n, -1)
    mu = F.linear(x, P['encoder.mu.weight'], P['encoder.mu.bias'])
    logvar = F.linear(x, P['encoder.logvar.weight'], P['encoder.logvar.bias'])
    z = mu + eps * torch.exp(0.5 * logvar)
    x = torch.cat([z, P['decoder.embedding.weight'].t()[lab]], 1)
    x = torch.relu(bn(F.linear(x, P['decoder.linear.0.weight'], P['decoder.linear.0.bias']), 'decoder.linear.1'))
    x = x.reshape(n, *shape)
    for r in range(nres):
        x = res(x, f'decoder.blocks.{r}')
    k = nres
    for _ in range(nstage - 1):
        q = f'decoder.blocks.{k}'
        x = torch.relu(bn(F.conv_transpose2d(x, P[q + '.weight'], P[q + '.bias'], stride=2, padding=1), f'decoder.blocks.{k + 1}'))
        k += 3
    q = f'decoder.blocks.{k}'
    logits = F.conv_transpose2d(x, P[q + '.weight'], P[q + '.bias'], stride=2, padding=1)
    bce = F.binary_cross_entropy_with_logits(logits, x01, reduction='sum')
    kld = 0.5 * torch.sum(mu.pow(2) + logvar.exp() - 1 - logvar)
    return (bce + kld) / img.numel()
