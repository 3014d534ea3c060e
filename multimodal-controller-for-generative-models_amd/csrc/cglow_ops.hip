// CGlow label-conditioned prior kernels (gfx950): the one place where the reference's CGlow (src/models/cglow.py) differs from
// MCGlow once the MultimodalControllers are gone.
//
//   Last block (no split): h = prior(zeros) + embedding(one_hot(label)) broadcast over H x W, mean | log_sd = h.chunk(2, 1)
//   (cglow.py:231-235, 254-258).  prior = ZeroConv2d(c, 2c, 3, 1, 1) on a zero input, embedding = ZeroConv2d(num_mode, 2c, 1, 1, 0)
//   on a one-hot input, ZeroConv2d(x) = (conv(x) + b) * exp(3 scale):
//     h[n][co] = b_p[co] * exp(3 s_p[co]) + (W_e[co][label_n] + b_e[co]) * exp(3 s_e[co]),   the same for every pixel.
//
// Forward: mcgen_cglow_prior writes the NHWC prior the Gaussian kernels (mcgen_gaussian_logp / _logp_bwd / _sample) read.
// Backward: mcgen_cglow_prior_bwd reduces the prior's gradient over the pixels to dh[n][co] and writes the gradients of both
// parameter sets; the table gradient dW_e[co][m] = sum_{label_n == m} dh[n][co] * exp(3 s_e[co]) is mcgen_cgan_embed_bwd over
// the scaled rows.  prior.conv.weight only ever multiplies zeros: its gradient is written as zero.
//
// Every reduction runs in a fixed order (pixels ascending, then samples ascending) with no float atomics: reruns and graph
// replays are bit-identical.  Labels outside [0, M) read a zero embedding row and write nothing.
#include "mcgen_common.h"

namespace {
#define STREAM(s) reinterpret_cast<hipStream_t>(s)

// out[n][p][c], pitch Cp: h[n][c] (c < C2), 0 after.  Grid (N, Y): the workgroup stages its sample's row in LDS once, then each
// thread writes 8 channels of a pixel with one 16-byte (bf16) or two 16-byte (fp32) stores.
template <typename T>
__global__ __launch_bounds__(256)
void prior_kernel(const float* __restrict__ b_p, const float* __restrict__ s_p, const float* __restrict__ w_e,
                  const float* __restrict__ b_e, const float* __restrict__ s_e, const int64_t* __restrict__ label,
                  T* __restrict__ out, int HW, int C2, int M, int Cp) {
    extern __shared__ float row[];      // [Cp]
    const int n = blockIdx.x;
    const int64_t m = label[n];
    const bool ok = m >= 0 && m < M;
    for (int c = threadIdx.x; c < Cp; c += blockDim.x) {
        float h = 0.f;
        if (c < C2) {
            const float e = ok ? w_e[(size_t)c * M + m] : 0.f;
            h = b_p[c] * expf(3.0f * s_p[c]) + (e + b_e[c]) * expf(3.0f * s_e[c]);
        }
        row[c] = h;
    }
    __syncthreads();
    const int cv = Cp / 8;
    const int total = HW * cv;
    T* o = out + (size_t)n * HW * Cp;
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < total; i += gridDim.y * blockDim.x) {
        const int p = i / cv, c0 = (i % cv) * 8;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = row[c0 + j];
        Elem<T>::store8(o + (size_t)p * Cp + c0, v);
    }
}

// dh[n][c] = sum_p dprior[n][p][c] (p ascending), de[n][c] = dh[n][c] * exp(3 s_e[c]).  Grid N, one thread per channel:
// consecutive threads read consecutive channels of a pixel.
template <typename T>
__global__ __launch_bounds__(256)
void prior_dh_kernel(const T* __restrict__ dprior, const float* __restrict__ s_e, float* __restrict__ dh, float* __restrict__ de,
                     int HW, int C2, int Cp) {
    const int n = blockIdx.x;
    const T* d = dprior + (size_t)n * HW * Cp;
    for (int c = threadIdx.x; c < C2; c += blockDim.x) {
        float s = 0.f;
        for (int p = 0; p < HW; ++p) s += Elem<T>::to_f(d[(size_t)p * Cp + c]);
        dh[(size_t)n * C2 + c] = s;
        de[(size_t)n * C2 + c] = s * expf(3.0f * s_e[c]);
    }
}

// Per channel c, n ascending:  S = sum_n dh[n][c],  Q = sum_n dh[n][c] * (W_e[c][label_n] + b_e[c])
//   db_p = S rp,  ds_p = 3 S b_p rp,  db_e = S re,  ds_e = 3 Q re   (rp = exp(3 s_p[c]), re = exp(3 s_e[c])).
// The labels are staged through LDS 1024 at a time.  Every thread of the grid then zeroes its stride of dw_p.
__global__ __launch_bounds__(256)
void prior_param_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ b_p, const float* __restrict__ s_p,
                            const float* __restrict__ w_e, const float* __restrict__ b_e, const float* __restrict__ s_e,
                            const int64_t* __restrict__ label, float* __restrict__ db_p, float* __restrict__ ds_p,
                            float* __restrict__ dw_p, int64_t dw_p_elems, float* __restrict__ db_e, float* __restrict__ ds_e,
                            int N, int C2, int M) {
    __shared__ int lab[1024];
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = c < C2;
    const float be = live ? b_e[c] : 0.f;
    float S = 0.f, Q = 0.f;
    for (int n0 = 0; n0 < N; n0 += 1024) {
        const int nn = min(1024, N - n0);
        __syncthreads();
        for (int k = threadIdx.x; k < nn; k += blockDim.x) {
            const int64_t l = label[n0 + k];
            lab[k] = (l >= 0 && l < M) ? (int)l : -1;
        }
        __syncthreads();
        if (live)
            for (int k = 0; k < nn; ++k) {
                const float g = dh[(size_t)(n0 + k) * C2 + c];
                const float e = lab[k] >= 0 ? w_e[(size_t)c * M + lab[k]] : 0.f;
                S += g;
                Q += g * (e + be);
            }
    }
    if (live) {
        const float rp = expf(3.0f * s_p[c]), re = expf(3.0f * s_e[c]);
        db_p[c] = S * rp;
        ds_p[c] = 3.0f * S * b_p[c] * rp;
        db_e[c] = S * re;
        ds_e[c] = 3.0f * Q * re;
    }
    if (dw_p)
        for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < dw_p_elems; i += (int64_t)gridDim.x * blockDim.x)
            dw_p[i] = 0.f;
}

inline int grid_for(size_t n, int block = 256, int cap = 65535) {
    size_t b = (n + block - 1) / block; if (b < 1) b = 1; if (b > (size_t)cap) b = cap; return (int)b;
}

#define DISPATCH_T(dtype, F32, BF16) \
    do { if ((dtype) == MCGEN_F32) { F32; } else if ((dtype) == MCGEN_BF16) { BF16; } else return mcgen_fail("bad dtype %d", (dtype)); } while (0)
}  // namespace

extern "C" int mcgen_cglow_prior(const float* b_p, const float* s_p, const float* w_e, const float* b_e, const float* s_e,
                                 const int64_t* label, void* out, int dtype, int N, int HW, int C2, int M, int Cp, void* stream) {
    MCGEN_CHECK(b_p && s_p && w_e && b_e && s_e && label && out && N > 0 && HW > 0 && C2 > 0 && C2 % 2 == 0 && M > 0 &&
                Cp >= C2 && Cp % 8 == 0 && Cp <= 8192,
                "cglow_prior: bad arguments (an even channel count C2; Cp >= C2, a multiple of 8, at most 8192)");
    MCGEN_CHECK(dtype == MCGEN_F32 || dtype == MCGEN_BF16, "cglow_prior: bad dtype %d", dtype);
    const size_t per_image = (size_t)HW * (Cp / 8);
    MCGEN_CHECK(per_image <= (size_t)1 << 30, "cglow_prior: map of %d pixels x %d channels is too large", HW, Cp);
    const dim3 grid(N, grid_for(per_image, 256, 8));
    const size_t lds = (size_t)Cp * sizeof(float);
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(prior_kernel<float>, grid, dim3(256), lds, STREAM(stream), b_p, s_p, w_e, b_e, s_e, label, (float*)out, HW, C2, M, Cp),
        hipLaunchKernelGGL(prior_kernel<bf16_t>, grid, dim3(256), lds, STREAM(stream), b_p, s_p, w_e, b_e, s_e, label, (bf16_t*)out, HW, C2, M, Cp));
    MCGEN_LAUNCH_CHECK("cglow_prior"); return 0;
}

extern "C" int mcgen_cglow_prior_bwd(const void* dprior, const float* b_p, const float* s_p, const float* w_e, const float* b_e,
                                     const float* s_e, const int64_t* label, float* workspace, float* db_p, float* ds_p,
                                     float* dw_p, int64_t dw_p_elems, float* dw_e, float* db_e, float* ds_e, int dtype, int N,
                                     int HW, int C2, int M, int Cp, void* stream) {
    MCGEN_CHECK(dprior && b_p && s_p && w_e && b_e && s_e && label && workspace && db_p && ds_p && dw_e && db_e && ds_e && N > 0 &&
                HW > 0 && C2 > 0 && C2 % 2 == 0 && M > 0 && Cp >= C2 && Cp % 8 == 0 && (dw_p ? dw_p_elems > 0 : dw_p_elems == 0),
                "cglow_prior_bwd: bad arguments (an even channel count C2; Cp >= C2, a multiple of 8; dw_p with its element count)");
    MCGEN_CHECK(dtype == MCGEN_F32 || dtype == MCGEN_BF16, "cglow_prior_bwd: bad dtype %d", dtype);
    float* dh = workspace;                      // [N][C2]
    float* de = workspace + (size_t)N * C2;     // [N][C2]: dh * exp(3 s_e), the rows of the table gradient
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(prior_dh_kernel<float>, dim3(N), dim3(256), 0, STREAM(stream), (const float*)dprior, s_e, dh, de, HW, C2, Cp),
        hipLaunchKernelGGL(prior_dh_kernel<bf16_t>, dim3(N), dim3(256), 0, STREAM(stream), (const bf16_t*)dprior, s_e, dh, de, HW, C2, Cp));
    MCGEN_LAUNCH_CHECK("cglow_prior_bwd");
    int blocks = (C2 + 255) / 256;              // the channels; up to 64 workgroups share the zero fill of dw_p
    if (dw_p && grid_for((size_t)dw_p_elems, 256, 64) > blocks) blocks = grid_for((size_t)dw_p_elems, 256, 64);
    hipLaunchKernelGGL(prior_param_bwd_kernel, dim3(blocks), dim3(256), 0, STREAM(stream), dh, b_p, s_p, w_e, b_e, s_e, label, db_p,
                       ds_p, dw_p, dw_p_elems, db_e, ds_e, N, C2, M);
    MCGEN_LAUNCH_CHECK("cglow_prior_bwd");
    return mcgen_cgan_embed_bwd(de, C2, label, dw_e, N, C2, M, 0, stream);
}
