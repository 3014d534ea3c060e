"""Float64 CPU references for the BCE branch of the GAN loop (cfg['loss_type'] = 'BCE', train_gan.py:148-152,168-170:
binary_cross_entropy_with_logits against ones and zeros, the non-saturating GAN loss), the error bounds the GPU tests of
csrc/small_ops.hip's BCE kernels hold them to, and the CPU oracle with the BCE loss lines.  test_gan_loss_ref_cpu.py checks
the references against torch's own float64 autograd; test_gan_loss_kernels_gpu.py and test_gan_bce_gpu.py use them.

Bounds (u = 2^-24; the assumptions are those of tests/test_pixel_vq_kernels_gpu.py's module docstring, which also records
the measured sigmoid error, 2.395 ulp on an MI355X):
- sigmoid q = 1 / (1 + expf(-a)) within 5u q; TINY = 2^-126 is added because expf overflows past 88.7 (q = 0 where the
  true value is a subnormal) and subnormal results may lose bits or flush.
- gradient d = +-q fl(1 / N): the sigmoid's 5u carried through 1 / N, the rounding of 1 / N and the product, 2u |d|;
  doubled for the second-order terms: 2 (5u q / N + 2u |d|) + TINY.
- softplus(a) = max(a, 0) + log1pf(expf(-|a|)) within (3 + 2 LOG1P_ULP) u softplus(a) + TINY, LOG1P_ULP = 2.
- loss = (sum of N terms) fl(1 / N) [+ the same]: the per-term bounds, then N - 1 additions, 1 / N, one product and the
  final addition, (N + 2) u sum terms; doubled: 2 (sum of per-term bounds + (N + 2) u sum terms) / N.
"""
import torch
import torch.nn.functional as F

from oracle import mcgan_oracle as O

F64 = torch.float64
U32 = 2.0 ** -24
TINY = 2.0 ** -126
LOG1P_ULP = 2
# exact 0; +-17: expf(-17) is below u, the sigmoid rounds to 1; +-88.8, +-100.5, +-200: expf overflows (past 88.72)
EXTREMES = [0.0, 1.0, -1.0, 17.0, -17.0, 88.8, -88.8, 100.5, -100.5, 200.0, -200.0]


def softplus(a):
    a = a.to(F64)
    return a.clamp_min(0.0) + torch.log1p(torch.exp(-a.abs()))


def sigmoid(a):
    """1 / (1 + exp(-a)) in float64 without overflow: exp(-|a|) only."""
    a = a.to(F64)
    e = torch.exp(-a.abs())
    return torch.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_d(real, fake):
    """train_gan.py:149-152: loss = mean softplus(-real) + mean softplus(fake) -> (loss, dreal = -sigmoid(-real) / N,
    dfake = sigmoid(fake) / N, loss_abs = the sum of the terms' magnitudes, already divided by N: every term is >= 0)."""
    real, fake = real.to(F64), fake.to(F64)
    n = real.numel()
    loss = softplus(-real).sum() / n + softplus(fake).sum() / n
    return loss, -sigmoid(-real) / n, sigmoid(fake) / n, loss


def bce_g(fake):
    """train_gan.py:169-170: loss = mean softplus(-fake) -> (loss, dfake = -sigmoid(-fake) / N, loss_abs)."""
    fake = fake.to(F64)
    n = fake.numel()
    loss = softplus(-fake).sum() / n
    return loss, -sigmoid(-fake) / n, loss


def grad_tol(d):
    """Bound of a gradient d = +-q / N (module docstring); q / N = |d|."""
    d = d.to(F64).abs()
    return 2 * (5 * U32 * d + 2 * U32 * d) + TINY


def loss_tol(terms, n):
    """Bound of loss = sum(terms) / N for the softplus terms `terms` (all of both sums, float64)."""
    terms = terms.to(F64)
    per_term = ((3 + 2 * LOG1P_ULP) * U32 * terms + TINY).sum()
    return 2 * (per_term + (n + 2) * U32 * terms.sum()) / n


def logits_with_extremes(n, *key):
    """N fp32 logits: random (scale 3) with every entry of EXTREMES at the front and, reversed, at the back -- past the
    first trip of a 256-thread loop where N > 256.  N < len(EXTREMES): the first N extremes (rotated by the key)."""
    import zlib
    gen = torch.Generator().manual_seed(zlib.crc32(repr((n,) + key).encode()) % 100003)
    x = torch.randn(n, generator=gen) * 3
    e = torch.tensor(EXTREMES)
    k = len(EXTREMES)
    if n >= 2 * k:
        x[:k], x[-k:] = e, e.flip(0)
    else:
        rot = int(torch.randint(0, k, (1,), generator=gen))
        x[:min(n, k)] = e.roll(rot)[:min(n, k)]
    return x


class OracleMCGANBCE(O.OracleMCGAN):
    """oracle.mcgan_oracle.OracleMCGAN with cfg['loss_type'] = 'BCE': `train_iteration` is the oracle's own with its two
    loss lines replaced by train_gan.py:149-152 and 169-170."""

    def train_iteration(self, img, label, zs):
        zi = iter(zs)
        n = img.size(0)
        for _ in range(self.d_iters):
            self._zero()
            d_x = self.discriminate(img, label)
            fake = self.generate(label, next(zi))
            d_gz = self.discriminate(fake.detach(), label)
            d_loss = F.binary_cross_entropy_with_logits(d_x, torch.ones((n, 1))) + \
                F.binary_cross_entropy_with_logits(d_gz, torch.zeros((n, 1)))
            d_loss.backward()
            self.opt_d.step()
        for _ in range(self.g_iters):
            self._zero()
            fake = self.generate(label, next(zi))
            g_loss = F.binary_cross_entropy_with_logits(self.discriminate(fake, label), torch.ones((n, 1)))
            g_loss.backward()
            self.opt_g.step()
        return float(d_loss.detach()), float(g_loss.detach())
