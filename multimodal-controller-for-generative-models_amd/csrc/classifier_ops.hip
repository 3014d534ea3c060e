// Classifier training kernels (gfx950): the backward of one block tail of models/classifier.py,
// y = MaxPool2d(2)(ReLU(BatchNorm2d(x))) with training-mode BatchNorm (classifier.py:17-29 in the reference).
//
// The forward of that tail is mcgen_affine_relu_maxpool2 with the batch affine sc = gamma * rstd, sh = beta - mean * sc.
// Its backward needs, per 2x2 window and channel, the position the max came from.  No index tensor is stored: both
// kernels re-read x (needed anyway for x_hat) and recompute r = relu(fma(x, sc, sh)) with the forward kernel's fp32
// arithmetic.  Tie rule (PyTorch's max_pool2d): the FIRST strict maximum in row-major window order (q = 0..3) gets the
// gradient; the ReLU gate (output > 0) then zeroes windows whose maximum is 0.  So dz = gp at the argmax if r_max > 0,
// dz = 0 everywhere else.
//
// Deterministic: per-block partial sums land in a fixed [blocks, 2, C] slab (reduced in block order by
// mcgen_bn_bwd_finalize), no float atomics, so reruns and graph replays give bit-identical gradients.
#include "mcgen_common.h"

namespace {
#define STREAM(s) reinterpret_cast<hipStream_t>(s)

inline int grid_for(size_t n, int block = 256, int cap = 4096) {
    size_t b = (n + block - 1) / block; if (b < 1) b = 1; if (b > (size_t)cap) b = cap; return (int)b;
}

// One pooled pixel x 8 channels: the window's four x vectors, and per channel the winning position (-1: no gradient).
template <typename T>
__device__ __forceinline__ void window_argmax(const T* __restrict__ x, size_t n, int ho, int wo, int Ho, int W, int C, int c,
                                              const float (&a)[8], const float (&b)[8], float (&xv)[4][8], int (&arg)[8]) {
    float best[8];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        Elem<T>::load8(x + (((n * 2 * Ho + 2 * ho + (q >> 1)) * W) + 2 * wo + (q & 1)) * C + c, xv[q]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        best[j] = fmaxf(fmaf(xv[0][j], a[j], b[j]), 0.f);
        arg[j] = 0;
    }
#pragma unroll
    for (int q = 1; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float r = fmaxf(fmaf(xv[q][j], a[j], b[j]), 0.f);
            if (r > best[j]) { best[j] = r; arg[j] = q; }
        }
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (!(best[j] > 0.f)) arg[j] = -1;
}

// pass 1: grid (blocks), 256 threads = `lanes` pooled pixels x C/8 channel groups; block b owns pooled pixels
// [b * ppb, (b + 1) * ppb).  part[b][0][c] = sum dz, part[b][1][c] = sum dz * x_hat over the block's windows.
template <typename T>
__global__ __launch_bounds__(256)
void maxpool2_bn_bwd_stats_kernel(const T* __restrict__ gp, const T* __restrict__ x, const float* __restrict__ sc,
                                  const float* __restrict__ sh, const float* __restrict__ mean, const float* __restrict__ rstd,
                                  float* __restrict__ part, int N, int Ho, int Wo, int C, size_t ppb) {
    const int cv = C / 8;
    const int lanes = 256 / cv;
    const int grp = threadIdx.x % cv, pl = threadIdx.x / cv;
    const int c = grp * 8;
    const int W = 2 * Wo;
    const size_t pooled = (size_t)N * Ho * Wo;
    const size_t p0 = blockIdx.x * ppb, p1 = (p0 + ppb < pooled) ? p0 + ppb : pooled;
    float a[8], b[8], mu[8], rs[8], s1[8], s2[8];
    load8f(sc + c, a); load8f(sh + c, b); load8f(mean + c, mu); load8f(rstd + c, rs);
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
    if (pl < lanes)
        for (size_t p = p0 + pl; p < p1; p += lanes) {
            const int wo = (int)(p % Wo); const size_t t = p / Wo;
            const int ho = (int)(t % Ho); const size_t n = t / Ho;
            float xv[4][8], g[8];
            int arg[8];
            window_argmax<T>(x, n, ho, wo, Ho, W, C, c, a, b, xv, arg);
            Elem<T>::load8(gp + p * C + c, g);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (arg[j] < 0) continue;
                float xs = xv[0][j];
#pragma unroll
                for (int q = 1; q < 4; ++q) xs = arg[j] == q ? xv[q][j] : xs;
                s1[j] += g[j];
                s2[j] += g[j] * ((xs - mu[j]) * rs[j]);
            }
        }
    __shared__ float red[256][17];
#pragma unroll
    for (int j = 0; j < 8; ++j) { red[threadIdx.x][j] = s1[j]; red[threadIdx.x][8 + j] = s2[j]; }
    __syncthreads();
    for (int cc = threadIdx.x; cc < 2 * C; cc += 256) {
        const int which = cc / C, ch = cc % C;
        float t = 0.f;
        for (int l = 0; l < lanes; ++l) t += red[l * cv + ch / 8][which * 8 + ch % 8];
        part[((size_t)blockIdx.x * 2 + which) * C + ch] = t;
    }
}

// pass 2: one thread per (pooled pixel, 8 channels) writes the four full-resolution positions of its window:
// dx = sc * (dz - sum dz / M - x_hat * sum (dz x_hat) / M), M = N * 2Ho * 2Wo.
template <typename T>
__global__ void maxpool2_bn_bwd_apply_kernel(const T* __restrict__ gp, const T* __restrict__ x, const float* __restrict__ sc,
                                             const float* __restrict__ sh, const float* __restrict__ mean,
                                             const float* __restrict__ rstd, const float* __restrict__ sums, float inv_count,
                                             T* __restrict__ dx, int N, int Ho, int Wo, int C) {
    const int cv = C / 8;
    const size_t total = (size_t)N * Ho * Wo * cv;
    const int W = 2 * Wo;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % cv) * 8; size_t t = i / cv;
        const int wo = (int)(t % Wo); t /= Wo;
        const int ho = (int)(t % Ho); const size_t n = t / Ho;
        float a[8], b[8], xv[4][8], g[8];
        int arg[8];
        load8f(sc + c, a); load8f(sh + c, b);
        window_argmax<T>(x, n, ho, wo, Ho, W, C, c, a, b, xv, arg);
        Elem<T>::load8(gp + (t * Wo + wo) * C + c, g);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float dz = arg[j] == q ? g[j] : 0.f;
                const float xh = (xv[q][j] - mean[c + j]) * rstd[c + j];
                o[j] = a[j] * (dz - sums[c + j] * inv_count - xh * sums[C + c + j] * inv_count);
            }
            Elem<T>::store8(dx + (((n * 2 * Ho + 2 * ho + (q >> 1)) * W) + 2 * wo + (q & 1)) * C + c, o);
        }
    }
}

#define DISPATCH_T(dtype, F32, BF16) \
    do { if ((dtype) == MCGEN_F32) { F32; } else if ((dtype) == MCGEN_BF16) { BF16; } else return mcgen_fail("bad dtype %d", (dtype)); } while (0)
}  // namespace

extern "C" int mcgen_maxpool2_bn_bwd_stats(const void* gp, const void* x, const float* scale, const float* shift, const float* mean,
                                           const float* rstd, float* partials, int blocks, int dtype, int N, int Ho, int Wo, int C,
                                           void* stream) {
    MCGEN_CHECK(gp && x && scale && shift && mean && rstd && partials && blocks > 0 && N > 0 && Ho > 0 && Wo > 0,
                "maxpool2_bn_bwd_stats: bad arguments");
    MCGEN_CHECK(C % 8 == 0 && C / 8 <= 256 && 256 % (C / 8) == 0, "maxpool2_bn_bwd_stats: C/8 must divide 256");
    const size_t pooled = (size_t)N * Ho * Wo;
    const size_t ppb = (pooled + blocks - 1) / blocks;
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(maxpool2_bn_bwd_stats_kernel<float>, dim3(blocks), dim3(256), 0, STREAM(stream), (const float*)gp, (const float*)x, scale, shift, mean, rstd, partials, N, Ho, Wo, C, ppb),
        hipLaunchKernelGGL(maxpool2_bn_bwd_stats_kernel<bf16_t>, dim3(blocks), dim3(256), 0, STREAM(stream), (const bf16_t*)gp, (const bf16_t*)x, scale, shift, mean, rstd, partials, N, Ho, Wo, C, ppb));
    MCGEN_LAUNCH_CHECK("maxpool2_bn_bwd_stats"); return 0;
}

extern "C" int mcgen_maxpool2_bn_bwd_apply(const void* gp, const void* x, const float* scale, const float* shift, const float* mean,
                                           const float* rstd, const float* sums, void* dx, int dtype, int N, int Ho, int Wo, int C,
                                           void* stream) {
    MCGEN_CHECK(gp && x && scale && shift && mean && rstd && sums && dx && N > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 8 == 0,
                "maxpool2_bn_bwd_apply: bad arguments (C a multiple of 8)");
    const size_t total = (size_t)N * Ho * Wo * (C / 8);
    const float inv = (float)(1.0 / ((double)N * 4.0 * Ho * Wo));
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(maxpool2_bn_bwd_apply_kernel<float>, dim3(grid_for(total)), dim3(256), 0, STREAM(stream), (const float*)gp, (const float*)x, scale, shift, mean, rstd, sums, inv, (float*)dx, N, Ho, Wo, C),
        hipLaunchKernelGGL(maxpool2_bn_bwd_apply_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, STREAM(stream), (const bf16_t*)gp, (const bf16_t*)x, scale, shift, mean, rstd, sums, inv, (bf16_t*)dx, N, Ho, Wo, C));
    MCGEN_LAUNCH_CHECK("maxpool2_bn_bwd_apply"); return 0;
}
