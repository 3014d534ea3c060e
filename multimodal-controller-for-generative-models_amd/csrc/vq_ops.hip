// VQ-VAE training kernels (gfx950): the training step of VectorQuantization (modules.py:18-43) and the MSE + tanh
// reconstruction loss of VQVAE.forward (vqvae.py:97-104).  Deterministic: no float atomics anywhere; every sum runs in
// a fixed order, so reruns and graph replays give bit-identical buffers.
//
// The EMA statistics sum_k = flatten^T @ onehot are a one-hot GEMM built on the fly: the pixels are split into fixed
// chunks of VQ_PC, and a workgroup owns (chunk, 64 codes).  Every lane (one code) walks every pixel of the chunk and adds
// the pixel's features when the code matches, branch-free, so a workgroup's time does not depend on the code histogram
// (with the reference initialisation nearly every pixel of the first steps picks one code).  The per-chunk slabs are
// summed in chunk order by the refresh kernel.
#include "mcgen_common.h"

namespace {
#define STREAM(s) reinterpret_cast<hipStream_t>(s)
constexpr int VQ_PC = 128;     // pixels per chunk (one statistics slab)
constexpr int VQ_KT = 64;      // codes per workgroup: one per lane
constexpr int VQ_DMAX = 64;    // embedding sizes up to 64: four waves x 16 features

inline int grid_for(size_t n, int block = 256, int cap = 4096) {
    size_t b = (n + block - 1) / block; if (b < 1) b = 1; if (b > (size_t)cap) b = cap; return (int)b;
}

// grid (chunks, train ? K / 64 : 1), 256 threads.
//  y == 0 : q[p] = E[:, k_p] (the codebook BEFORE this step's update), g[p] = coef * (f[p] - q[p]) (optional),
//           dpart[chunk] = sum over the chunk of (q - f)^2
//  train  : cslab[chunk][k] = #{p in chunk : k_p = k}, slab[chunk][d][k] = sum_{p in chunk, k_p = k} f[p][d]
template <typename T>
__global__ __launch_bounds__(256)
void vq_stats_kernel(const float* __restrict__ f, const int64_t* __restrict__ idx, const float* __restrict__ emb,
                     T* __restrict__ q, T* __restrict__ g, float* __restrict__ slab, float* __restrict__ cslab,
                     float* __restrict__ dpart, float coef, int P, int D, int Fp, int K, int train) {
    __shared__ __attribute__((aligned(16))) float fs[VQ_PC * VQ_DMAX];
    __shared__ int ks[VQ_PC];
    __shared__ float red[4];
    const int chunk = blockIdx.x, p0 = chunk * VQ_PC;
    const int np = min(VQ_PC, P - p0);
    const int tid = threadIdx.x, d8n = D / 8;
    for (int i = tid; i < np * d8n; i += 256) {
        const int p = i / d8n, d = (i - p * d8n) * 8;
        float v[8];
        load8f(f + (size_t)(p0 + p) * Fp + d, v);
        *reinterpret_cast<f32x4*>(&fs[p * D + d]) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(&fs[p * D + d + 4]) = f32x4{v[4], v[5], v[6], v[7]};
    }
    for (int i = tid; i < np; i += 256) ks[i] = (int)idx[p0 + i];
    __syncthreads();
    if (blockIdx.y == 0) {
        float s = 0.f;
        for (int i = tid; i < np * d8n; i += 256) {
            const int p = i / d8n, d = (i - p * d8n) * 8;
            const int k = ks[p];
            float qv[8], gv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                qv[j] = emb[(size_t)(d + j) * K + k];
                const float e = fs[p * D + d + j] - qv[j];
                s += e * e;
                gv[j] = coef * e;
            }
            Elem<T>::store8(q + (size_t)(p0 + p) * D + d, qv);
            if (g) Elem<T>::store8(g + (size_t)(p0 + p) * D + d, gv);
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) dpart[chunk] = (red[0] + red[1]) + (red[2] + red[3]);
    }
    if (!train) return;
    const int lane = tid & 63, wave = tid >> 6;
    const int k = blockIdx.y * VQ_KT + lane;
    const int d0 = wave * 16;
    if (d0 >= D) return;                                        // (D < 64: the upper waves have no features)
    float acc[16], cnt = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    if (d0 + 16 <= D) {
        for (int p = 0; p < np; ++p) {
            const float m = (ks[p] == k) ? 1.f : 0.f;
            const f32x4* row = reinterpret_cast<const f32x4*>(&fs[p * D + d0]);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f32x4 v = row[c];
                acc[4 * c + 0] += m * v[0]; acc[4 * c + 1] += m * v[1];
                acc[4 * c + 2] += m * v[2]; acc[4 * c + 3] += m * v[3];
            }
            cnt += m;
        }
    } else {                                                    // D = 8 .. 56 not a multiple of 16: the last wave's part
        const int nd = D - d0;
        for (int p = 0; p < np; ++p) {
            const float m = (ks[p] == k) ? 1.f : 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < nd) acc[j] += m * fs[p * D + d0 + j];
            cnt += m;
        }
    }
    const int nd = min(16, D - d0);
    float* out = slab + (size_t)chunk * D * K + k;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < nd) out[(size_t)(d0 + j) * K] = acc[j];
    if (wave == 0) cslab[(size_t)chunk * K + k] = cnt;
}

// one workgroup: count_k = sum over chunks (chunk order), cluster_size <- decay * cluster_size + (1 - decay) * count,
// n = sum_k cluster_size (fixed tree), cs_k = (cluster_size_k + eps) / (n + K eps) * n;  diff = sum(dpart) / (P D)
__global__ __launch_bounds__(1024)
void vq_count_kernel(const float* __restrict__ cslab, const float* __restrict__ dpart, int chunks, int K, float decay,
                     float one_m_decay, float eps, float inv_numel, float* __restrict__ cluster_size, float* __restrict__ counts,
                     float* __restrict__ cs_out, float* __restrict__ diff, int train) {
    __shared__ float red[16];
    __shared__ float nsh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float part = 0.f;
    for (int k = tid; k < K && train; k += 1024) {
        float c = 0.f;
        for (int s = 0; s < chunks; ++s) c += cslab[(size_t)s * K + k];
        const float v = decay * cluster_size[k] + one_m_decay * c;
        cluster_size[k] = v;
        if (counts) counts[k] = c;
        part += v;
    }
    for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (tid == 0) {
        float n = 0.f;
        for (int w = 0; w < 16; ++w) n += red[w];
        nsh = n;
        float dsum = 0.f;
        for (int s = 0; s < chunks; ++s) dsum += dpart[s];
        *diff = dsum * inv_numel;
    }
    __syncthreads();
    if (!train) return;
    const float n = nsh, den = n + (float)K * eps;
    for (int k = tid; k < K; k += 1024) cs_out[k] = (cluster_size[k] + eps) / den * n;
}

// embedding_mean <- decay * embedding_mean + (1 - decay) * sum (chunk order);  embedding = embedding_mean / cs
__global__ __launch_bounds__(256)
void vq_refresh_kernel(const float* __restrict__ slab, const float* __restrict__ cs, int chunks, int D, int K, float decay,
                       float one_m_decay, float* __restrict__ emb_mean, float* __restrict__ emb) {
    const size_t total4 = (size_t)D * K / 4, stride = (size_t)D * K;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < chunks; ++c) s += *reinterpret_cast<const f32x4*>(slab + c * stride + 4 * i);
        const int k = (int)((4 * i) % K);
        const f32x4 m0 = *reinterpret_cast<const f32x4*>(emb_mean + 4 * i);
        const f32x4 c4 = *reinterpret_cast<const f32x4*>(cs + k);
        f32x4 m, e;
#pragma unroll
        for (int j = 0; j < 4; ++j) { m[j] = decay * m0[j] + one_m_decay * s[j]; e[j] = m[j] / c4[j]; }
        *reinterpret_cast<f32x4*>(emb_mean + 4 * i) = m;
        *reinterpret_cast<f32x4*>(emb + 4 * i) = e;
    }
}

// decoded = tanh(x); part[block] = sum (decoded - t)^2; dx = gscale * (decoded - t) * (1 - decoded^2)  (8 channels per lane)
template <typename T>
__global__ __launch_bounds__(256)
void mse_tanh_kernel(const T* __restrict__ x, const float* __restrict__ t, T* __restrict__ dec, T* __restrict__ dx,
                     float* __restrict__ part, float gscale, size_t pixels, int C, int Cp) {
    __shared__ float red[4];
    const int cv = Cp / 8;
    const size_t total = pixels * cv;
    float s = 0.f;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % cv) * 8;
        float xv[8], tv[8], r[8], d[8];
        Elem<T>::load8(x + i * 8, xv);
        load8f(t + i * 8, tv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            r[j] = 0.f; d[j] = 0.f;
            if (c0 + j < C) {
                r[j] = tanhf(xv[j]);
                const float e = r[j] - tv[j];
                s += e * e;
                d[j] = gscale * e * (1.f - r[j] * r[j]);
            }
        }
        Elem<T>::store8(dec + i * 8, r);
        if (dx) Elem<T>::store8(dx + i * 8, d);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace

#define DISPATCH_T(dtype, CALL_F32, CALL_BF16) \
    if (dtype == MCGEN_F32) { CALL_F32; } else if (dtype == MCGEN_BF16) { CALL_BF16; } \
    else return mcgen_fail("unknown dtype %d", dtype)

extern "C" int mcgen_vq_chunks(int64_t pixels) {
    return pixels > 0 ? (int)((pixels + VQ_PC - 1) / VQ_PC) : 0;
}

extern "C" int mcgen_vq_stats(const float* feat, const int64_t* idx, const float* embedding, void* q, void* g, float* slab,
                              float* cslab, float* dpart, float coef, int dtype, int64_t pixels, int D, int Fp, int K, int train,
                              void* stream) {
    MCGEN_CHECK(feat && idx && embedding && q && dpart && pixels > 0 && pixels < (1ll << 30), "vq_stats: bad arguments");
    MCGEN_CHECK(D > 0 && D % 8 == 0 && D <= VQ_DMAX && Fp >= D && Fp % 8 == 0, "vq_stats: D must be a multiple of 8 up to %d", VQ_DMAX);
    MCGEN_CHECK(K > 0 && K % VQ_KT == 0, "vq_stats: K must be a multiple of %d", VQ_KT);
    MCGEN_CHECK(!train || (slab && cslab), "vq_stats: training needs the statistics slabs");
    const int chunks = mcgen_vq_chunks(pixels);
    const dim3 grid(chunks, train ? K / VQ_KT : 1);
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(vq_stats_kernel<float>, grid, dim3(256), 0, STREAM(stream), feat, idx, embedding, (float*)q, (float*)g, slab, cslab, dpart, coef, (int)pixels, D, Fp, K, train),
        hipLaunchKernelGGL(vq_stats_kernel<bf16_t>, grid, dim3(256), 0, STREAM(stream), feat, idx, embedding, (bf16_t*)q, (bf16_t*)g, slab, cslab, dpart, coef, (int)pixels, D, Fp, K, train));
    MCGEN_LAUNCH_CHECK("vq_stats"); return 0;
}

extern "C" int mcgen_vq_update(const float* slab, const float* cslab, const float* dpart, int64_t pixels, int D, int K, float decay,
                               float one_m_decay, float eps, float* cluster_size, float* embedding_mean, float* embedding,
                               float* counts, float* cs_scratch, float* diff, int train, void* stream) {
    MCGEN_CHECK(dpart && diff && pixels > 0 && D > 0 && D % 8 == 0 && K > 0 && K % VQ_KT == 0, "vq_update: bad arguments");
    MCGEN_CHECK(!train || (slab && cslab && cluster_size && embedding_mean && embedding && cs_scratch), "vq_update: training needs the buffers");
    const int chunks = mcgen_vq_chunks(pixels);
    const float inv = (float)(1.0 / ((double)pixels * D));
    hipLaunchKernelGGL(vq_count_kernel, dim3(1), dim3(1024), 0, STREAM(stream), cslab, dpart, chunks, K, decay, one_m_decay, eps, inv,
                       cluster_size, counts, cs_scratch, diff, train);
    MCGEN_LAUNCH_CHECK("vq_count");
    if (!train) return 0;
    hipLaunchKernelGGL(vq_refresh_kernel, dim3(grid_for((size_t)D * K / 4)), dim3(256), 0, STREAM(stream), slab, cs_scratch, chunks, D, K,
                       decay, one_m_decay, embedding_mean, embedding);
    MCGEN_LAUNCH_CHECK("vq_refresh"); return 0;
}

extern "C" int mcgen_mse_tanh(const void* x, const float* target, void* decoded, void* dx, float* partials, int blocks, float gscale,
                              int dtype, int64_t pixels, int C, int Cp, void* stream) {
    MCGEN_CHECK(x && target && decoded && partials && blocks > 0 && blocks <= 4096 && pixels > 0 && C > 0 && Cp >= C && Cp % 8 == 0,
                "mse_tanh: bad arguments");
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(mse_tanh_kernel<float>, dim3(blocks), dim3(256), 0, STREAM(stream), (const float*)x, target, (float*)decoded, (float*)dx, partials, gscale, (size_t)pixels, C, Cp),
        hipLaunchKernelGGL(mse_tanh_kernel<bf16_t>, dim3(blocks), dim3(256), 0, STREAM(stream), (const bf16_t*)x, target, (bf16_t*)decoded, (bf16_t*)dx, partials, gscale, (size_t)pixels, C, Cp));
    MCGEN_LAUNCH_CHECK("mse_tanh"); return 0;
}
