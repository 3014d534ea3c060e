// CPixelCNN-specific kernels (gfx950): the conditional gated activation of ConditionalGatedMaskedConv2d, whose two gates
// read s + E[label_n] (E = class_cond_embedding.weight [M][2C] fp32, one row per sample, added in the kernel so that the
// stored h_vert / s stay unbiased: vert_to_horiz reads h_vert without the row), the BatchNorm statistics of that biased
// input, the backward through the batch statistics with per-image sums of the input gradient, the per-label embedding
// gradient, and the per-sample row gather of the incremental sampler.
// Every reduction runs in a fixed order with no float atomics.  Gathers clamp a label into [0, M); the embedding gradient
// skips a label outside it.  Reference: models/cpixelcnn.py (entry points documented in include/mcgen_hip.h).
#include "mcgen_common.h"

namespace {
#define STREAM(s) reinterpret_cast<hipStream_t>(s)
inline int grid_for(size_t n, int block = 256, int cap = 4096) {
    size_t b = (n + block - 1) / block; if (b < 1) b = 1; if (b > (size_t)cap) b = cap; return (int)b;
}
__device__ __forceinline__ int clamp_label(int64_t v, int M) { return v < 0 ? 0 : (v >= M ? M - 1 : (int)v); }

// the 2C-channel row of sample n, channels c .. c+7 of the first half and of the second half
__device__ __forceinline__ const float* row_of(const float* table, const int64_t* label, int M, size_t n, int C) {
    return table + (size_t)clamp_label(label[n], M) * 2 * C;
}

struct CGateJobs { mcgen_cgate_t j[MCGEN_CGATE_MAX]; };

// ---- BatchNorm statistics of a = s[:, :C] + e[:C]: per-block (sum a, sum a^2) in the conv-epilogue layout [blocks][2][C] ----
template <typename T>
__global__ __launch_bounds__(256) void cgate_stats_kernel(const CGateJobs jobs) {
    const mcgen_cgate_t& J = jobs.j[blockIdx.y];
    if ((int)blockIdx.x >= J.blocks) return;                     // (workgroup-uniform)
    const int C = J.C, cv = C / 8, lanes = 256 / cv;
    const int grp = threadIdx.x % cv, pl = threadIdx.x / cv, c = grp * 8;
    const size_t pixels = (size_t)J.N * J.HW, ppb = (pixels + J.blocks - 1) / J.blocks;
    const size_t p0 = blockIdx.x * ppb, p1 = (p0 + ppb < pixels) ? p0 + ppb : pixels;
    const T* s = reinterpret_cast<const T*>(J.s);
    float s1[8], s2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { s1[k] = 0.f; s2[k] = 0.f; }
    if (pl < lanes)
        for (size_t p = p0 + pl; p < p1; p += lanes) {
            float a[8], e[8];
            Elem<T>::load8(s + p * 2 * C + c, a);
            load8f(row_of(J.table, J.label, J.M, p / J.HW, C) + c, e);
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float x = a[k] + e[k]; s1[k] += x; s2[k] += x * x; }
        }
    __shared__ float red[256][17];
#pragma unroll
    for (int k = 0; k < 8; ++k) { red[threadIdx.x][k] = s1[k]; red[threadIdx.x][8 + k] = s2[k]; }
    __syncthreads();
    for (int cc = threadIdx.x; cc < 2 * C; cc += 256) {
        const int which = cc / C, ch = cc % C;
        float t = 0.f;
        for (int l = 0; l < lanes; ++l) t += red[l * cv + ch / 8][which * 8 + ch % 8];
        J.partials[((size_t)blockIdx.x * 2 + which) * C + ch] = t;
    }
}

// ---- forward: out = relu((a + e_a) * sc + sh) * sigmoid(b + e_b) ----------------------------------------------------------
template <typename T>
__global__ void cgated_fwd_kernel(const CGateJobs jobs) {
    const mcgen_cgate_t& J = jobs.j[blockIdx.y];
    const int C = J.C, cv = C / 8;
    const size_t total = (size_t)J.N * J.HW * cv;
    const T* s = reinterpret_cast<const T*>(J.s);
    T* out = reinterpret_cast<T*>(J.out);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % cv) * 8; const size_t p = i / cv;
        const float* e = row_of(J.table, J.label, J.M, p / J.HW, C);
        float a[8], b[8], ea[8], eb[8], o[8];
        Elem<T>::load8(s + p * 2 * C + c, a);
        Elem<T>::load8(s + p * 2 * C + C + c, b);
        load8f(e + c, ea);
        load8f(e + C + c, eb);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float z = fmaf(a[k] + ea[k], J.scale[c + k], J.shift[c + k]);
            o[k] = fmaxf(z, 0.f) / (1.f + expf(-(b[k] + eb[k])));
        }
        Elem<T>::store8(out + p * C + c, o);
    }
}

// ---- backward pass 1: ds[:, :C] = dz = g * q * [z > 0], ds[:, C:] = g * relu(z) * q * (1 - q), q = sigmoid(b + e_b);
// per-block partial sums of dz and dz * xhat (xhat = (a + e_a - mean) * rstd), layout [blocks][2][C] ----------------------
template <typename T>
__global__ __launch_bounds__(256)
void cgated_bwd_stats_kernel(const T* __restrict__ s, const float* __restrict__ table, const int64_t* __restrict__ label, int M,
                             const float* __restrict__ sc, const float* __restrict__ sh, const float* __restrict__ mean,
                             const float* __restrict__ rstd, const T* __restrict__ g, T* __restrict__ ds, float* __restrict__ part,
                             size_t pixels, int HW, int C, size_t ppb) {
    const int cv = C / 8, lanes = 256 / cv;
    const int grp = threadIdx.x % cv, pl = threadIdx.x / cv, c = grp * 8;
    const size_t p0 = blockIdx.x * ppb, p1 = (p0 + ppb < pixels) ? p0 + ppb : pixels;
    float s1[8], s2[8], scv[8], shv[8], mv[8], rv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { s1[k] = 0.f; s2[k] = 0.f; scv[k] = sc[c + k]; shv[k] = sh[c + k]; mv[k] = mean[c + k]; rv[k] = rstd[c + k]; }
    if (pl < lanes)
        for (size_t p = p0 + pl; p < p1; p += lanes) {
            const float* e = row_of(table, label, M, p / HW, C);
            float a[8], b[8], ea[8], eb[8], gv[8], dz[8], db[8];
            Elem<T>::load8(s + p * 2 * C + c, a);
            Elem<T>::load8(s + p * 2 * C + C + c, b);
            Elem<T>::load8(g + p * C + c, gv);
            load8f(e + c, ea);
            load8f(e + C + c, eb);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float x = a[k] + ea[k];
                const float z = fmaf(x, scv[k], shv[k]);
                const float q = 1.f / (1.f + expf(-(b[k] + eb[k])));
                dz[k] = z > 0.f ? gv[k] * q : 0.f;
                db[k] = gv[k] * fmaxf(z, 0.f) * q * (1.f - q);
                s1[k] += dz[k];
                s2[k] += dz[k] * ((x - mv[k]) * rv[k]);
            }
            Elem<T>::store8(ds + p * 2 * C + c, dz);
            Elem<T>::store8(ds + p * 2 * C + C + c, db);
        }
    __shared__ float red[256][17];
#pragma unroll
    for (int k = 0; k < 8; ++k) { red[threadIdx.x][k] = s1[k]; red[threadIdx.x][8 + k] = s2[k]; }
    __syncthreads();
    for (int cc = threadIdx.x; cc < 2 * C; cc += 256) {
        const int which = cc / C, ch = cc % C;
        float t = 0.f;
        for (int l = 0; l < lanes; ++l) t += red[l * cv + ch / 8][which * 8 + ch % 8];
        part[((size_t)blockIdx.x * 2 + which) * C + ch] = t;
    }
}

// ---- backward pass 2, one workgroup per image: da = sc * (dz - (S1 + xhat * S2) / count) in place on ds[:, :C], and
// dsum[n][ch] = sum over the image's pixels (ascending) of ds[n, p, ch] for all 2C channels (da before its rounding) --------
template <typename T>
__global__ __launch_bounds__(256)
void cgated_bwd_apply_kernel(T* __restrict__ ds, const T* __restrict__ s, const float* __restrict__ table,
                             const int64_t* __restrict__ label, int M, const float* __restrict__ sums, const float* __restrict__ sc,
                             const float* __restrict__ mean, const float* __restrict__ rstd, float inv_count,
                             float* __restrict__ dsum, int HW, int C) {
    const size_t n = blockIdx.x;
    const int C2 = 2 * C;
    const float* e = row_of(table, label, M, n, C);
    for (int ch = threadIdx.x; ch < C2; ch += blockDim.x) {
        float acc = 0.f;
        if (ch < C) {
            const float ec = e[ch], m = mean[ch], r = rstd[ch], k = sc[ch], S1 = sums[ch], S2 = sums[C + ch];
            for (int p = 0; p < HW; ++p) {
                const size_t o = (n * HW + p) * C2 + ch;
                const float xh = (Elem<T>::to_f(s[o]) + ec - m) * r;
                const float da = k * (Elem<T>::to_f(ds[o]) - (S1 + xh * S2) * inv_count);
                ds[o] = Elem<T>::from_f(da);
                acc += da;
            }
        } else {
            for (int p = 0; p < HW; ++p) acc += Elem<T>::to_f(ds[(n * HW + p) * C2 + ch]);
        }
        dsum[n * C2 + ch] = acc;
    }
}

// ---- dE[m][c] = sum over n ascending with label_n == m of (dsum_v[n][c] + dsum_h[n][c]); absent modes 0 -------------------
__global__ void cpx_embed_bwd_kernel(const float* __restrict__ dsum_v, const float* __restrict__ dsum_h,
                                     const int64_t* __restrict__ label, float* __restrict__ dE, int N, int C2, int M) {
    const size_t total = (size_t)M * C2;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C2); const int64_t m = (int64_t)(i / C2);
        float acc = 0.f;
        for (int n = 0; n < N; ++n) {
            if (label[n] != m) continue;
            const float h = dsum_h[(size_t)n * C2 + c];
            acc += dsum_v ? dsum_v[(size_t)n * C2 + c] + h : h;
        }
        dE[i] = acc;
    }
}

// ---- out[l][n][:] = tables[l][clamp(label_n)][:] --------------------------------------------------------------------------
__global__ void cpx_gather_rows_kernel(const float* __restrict__ tables, const int64_t* __restrict__ label, float* __restrict__ out,
                                       int L, int N, int C2, int M) {
    const size_t total = (size_t)L * N * C2;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C2); const size_t r = i / C2;
        const int n = (int)(r % N), l = (int)(r / N);
        out[i] = tables[((size_t)l * M + clamp_label(label[n], M)) * C2 + c];
    }
}

// ---- dE[k][c] = sum over pixels p ascending with codes[p] == k of dx[p][c]: the code embedding's gradient in a fixed order.
// One workgroup per code: each 256-pixel chunk's matches are compacted into LDS in ascending order (wave ballots), then
// thread c adds their rows.  Codes outside [0, K) match no workgroup. ---------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256)
void code_embed_bwd_kernel(const T* __restrict__ dx, int Cp, const int64_t* __restrict__ codes, float* __restrict__ dE,
                           size_t P, int C) {
    __shared__ int list[256];
    __shared__ int wc[4];
    const int64_t k = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float acc = 0.f;
    for (size_t base = 0; base < P; base += 256) {
        const size_t p = base + tid;
        const bool match = p < P && codes[p] == k;
        const unsigned long long b = __ballot(match);
        if (lane == 0) wc[wave] = __popcll(b);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < 4; ++w) { if (w < wave) off += wc[w]; total += wc[w]; }
        if (match) list[off + __popcll(b & ((1ull << lane) - 1ull))] = (int)(p - base);
        __syncthreads();
        if (tid < C)
            for (int i = 0; i < total; ++i) acc += Elem<T>::to_f(dx[(base + list[i]) * Cp + tid]);
        __syncthreads();                                  // list / wc are rewritten by the next chunk
    }
    if (tid < C) dE[(size_t)k * C + tid] = acc;
}

int check_jobs(const mcgen_cgate_t* jobs, int n, bool fwd, CGateJobs& t, const char* what) {
    MCGEN_CHECK(jobs && n >= 1 && n <= MCGEN_CGATE_MAX, "%s: 1 .. %d gates", what, MCGEN_CGATE_MAX);
    for (int i = 0; i < n; ++i) {
        const mcgen_cgate_t& j = jobs[i];
        MCGEN_CHECK(j.s && j.table && j.label && j.N > 0 && j.HW > 0 && j.M > 0 && j.C > 0 && j.C % 8 == 0, "%s: bad job %d", what, i);
        if (fwd) MCGEN_CHECK(j.scale && j.shift && j.out, "%s: job %d needs scale, shift and out", what, i);
        else MCGEN_CHECK(j.partials && j.blocks > 0 && j.C / 8 <= 256 && 256 % (j.C / 8) == 0,
                         "%s: job %d needs partials, blocks > 0 and C/8 dividing 256", what, i);
        t.j[i] = j;
    }
    for (int i = n; i < MCGEN_CGATE_MAX; ++i) t.j[i] = jobs[0];
    return 0;
}
}  // namespace

#define DISPATCH_T(dtype, F32, BF16) \
    do { if ((dtype) == MCGEN_F32) { F32; } else if ((dtype) == MCGEN_BF16) { BF16; } else return mcgen_fail("bad dtype %d", (dtype)); } while (0)

extern "C" int mcgen_cpx_gate_stats(const mcgen_cgate_t* jobs, int n, int dtype, void* stream) {
    CGateJobs t;
    if (int rc = check_jobs(jobs, n, false, t, "cpx_gate_stats")) return rc;
    int most = 1;
    for (int i = 0; i < n; ++i) if (jobs[i].blocks > most) most = jobs[i].blocks;
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(cgate_stats_kernel<float>, dim3(most, n), dim3(256), 0, STREAM(stream), t),
        hipLaunchKernelGGL(cgate_stats_kernel<bf16_t>, dim3(most, n), dim3(256), 0, STREAM(stream), t));
    MCGEN_LAUNCH_CHECK("cpx_gate_stats"); return 0;
}

extern "C" int mcgen_cpx_gated_fwd(const mcgen_cgate_t* jobs, int n, int dtype, void* stream) {
    CGateJobs t;
    if (int rc = check_jobs(jobs, n, true, t, "cpx_gated_fwd")) return rc;
    size_t most = 1;
    for (int i = 0; i < n; ++i) {
        const size_t total = (size_t)jobs[i].N * jobs[i].HW * (jobs[i].C / 8);
        if (total > most) most = total;
    }
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(cgated_fwd_kernel<float>, dim3(grid_for(most), n), dim3(256), 0, STREAM(stream), t),
        hipLaunchKernelGGL(cgated_fwd_kernel<bf16_t>, dim3(grid_for(most), n), dim3(256), 0, STREAM(stream), t));
    MCGEN_LAUNCH_CHECK("cpx_gated_fwd"); return 0;
}

extern "C" int mcgen_cpx_gated_bwd_stats(const void* s, const float* table, const int64_t* label, int M, const float* scale,
                                         const float* shift, const float* mean, const float* rstd, const void* g, void* ds,
                                         float* partials, int blocks, int dtype, int N, int HW, int C, void* stream) {
    MCGEN_CHECK(s && table && label && M > 0 && scale && shift && mean && rstd && g && ds && partials && blocks > 0 && N > 0 && HW > 0,
                "cpx_gated_bwd_stats: bad arguments");
    MCGEN_CHECK(C % 8 == 0 && C / 8 <= 256 && 256 % (C / 8) == 0, "cpx_gated_bwd_stats: C/8 must divide 256");
    const size_t pixels = (size_t)N * HW, ppb = (pixels + blocks - 1) / blocks;
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(cgated_bwd_stats_kernel<float>, dim3(blocks), dim3(256), 0, STREAM(stream), (const float*)s, table, label, M,
                           scale, shift, mean, rstd, (const float*)g, (float*)ds, partials, pixels, HW, C, ppb),
        hipLaunchKernelGGL(cgated_bwd_stats_kernel<bf16_t>, dim3(blocks), dim3(256), 0, STREAM(stream), (const bf16_t*)s, table, label, M,
                           scale, shift, mean, rstd, (const bf16_t*)g, (bf16_t*)ds, partials, pixels, HW, C, ppb));
    MCGEN_LAUNCH_CHECK("cpx_gated_bwd_stats"); return 0;
}

extern "C" int mcgen_cpx_gated_bwd_apply(void* ds, const void* s, const float* table, const int64_t* label, int M, const float* sums,
                                         const float* scale, const float* mean, const float* rstd, double count, float* dsum,
                                         int dtype, int N, int HW, int C, void* stream) {
    MCGEN_CHECK(ds && s && table && label && M > 0 && sums && scale && mean && rstd && dsum && count > 0 && N > 0 && HW > 0 && C % 8 == 0,
                "cpx_gated_bwd_apply: bad arguments");
    const float inv = (float)(1.0 / count);
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(cgated_bwd_apply_kernel<float>, dim3(N), dim3(256), 0, STREAM(stream), (float*)ds, (const float*)s, table, label,
                           M, sums, scale, mean, rstd, inv, dsum, HW, C),
        hipLaunchKernelGGL(cgated_bwd_apply_kernel<bf16_t>, dim3(N), dim3(256), 0, STREAM(stream), (bf16_t*)ds, (const bf16_t*)s, table,
                           label, M, sums, scale, mean, rstd, inv, dsum, HW, C));
    MCGEN_LAUNCH_CHECK("cpx_gated_bwd_apply"); return 0;
}

extern "C" int mcgen_cpx_embed_bwd(const float* dsum_v, const float* dsum_h, const int64_t* label, float* dE, int N, int C2, int M,
                                   void* stream) {
    MCGEN_CHECK(dsum_h && label && dE && N > 0 && C2 > 0 && M > 0, "cpx_embed_bwd: bad arguments");
    hipLaunchKernelGGL(cpx_embed_bwd_kernel, dim3(grid_for((size_t)M * C2)), dim3(256), 0, STREAM(stream), dsum_v, dsum_h, label, dE, N,
                       C2, M);
    MCGEN_LAUNCH_CHECK("cpx_embed_bwd"); return 0;
}

extern "C" int mcgen_cpx_gather_rows(const float* tables, const int64_t* label, float* out, int L, int N, int C2, int M, void* stream) {
    MCGEN_CHECK(tables && label && out && L > 0 && N > 0 && C2 > 0 && M > 0, "cpx_gather_rows: bad arguments");
    hipLaunchKernelGGL(cpx_gather_rows_kernel, dim3(grid_for((size_t)L * N * C2)), dim3(256), 0, STREAM(stream), tables, label, out, L, N,
                       C2, M);
    MCGEN_LAUNCH_CHECK("cpx_gather_rows"); return 0;
}

extern "C" int mcgen_cpx_code_embed_bwd(const void* dx, int Cp, const int64_t* codes, float* dE, int64_t P, int K, int C, int dtype,
                                        void* stream) {
    MCGEN_CHECK(dx && codes && dE && P > 0 && K > 0 && C > 0 && C <= 256 && Cp >= C, "cpx_code_embed_bwd: bad arguments");
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(code_embed_bwd_kernel<float>, dim3(K), dim3(256), 0, STREAM(stream), (const float*)dx, Cp, codes, dE,
                           (size_t)P, C),
        hipLaunchKernelGGL(code_embed_bwd_kernel<bf16_t>, dim3(K), dim3(256), 0, STREAM(stream), (const bf16_t*)dx, Cp, codes, dE,
                           (size_t)P, C));
    MCGEN_LAUNCH_CHECK("cpx_code_embed_bwd"); return 0;
}
