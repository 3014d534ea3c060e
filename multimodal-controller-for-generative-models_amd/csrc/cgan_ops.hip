// CGAN label-embedding kernels (gfx950): the two places where the reference's CGAN (src/models/cgan.py) differs from MCGAN
// once the MultimodalControllers are gone.
//
//   Generator:     x = cat(z, embedding(one_hot(label)))          -> Linear(latent + E, 16 C0)   (cgan.py:57-60)
//                  embedding(one_hot(label)) = W[:, label], W = embedding.weight [E, M]
//   Discriminator: x = cat(img, (W / sigma)[:, label] broadcast over H x W) -> FirstDisResBlock  (cgan.py:166-170)
//
// Forward: mcgen_cgan_gen_input writes the generator's Linear input rows [z (+) W[:, label] (+) 0]; mcgen_cgan_dis_input
// writes the discriminator's input image with the embedding channels appended.  Backward: the embedding's gradient
// dW[:, m] = sum over the samples n with label_n == m of dE[n] (mcgen_cgan_embed_bwd); dE comes from
//   * the generator's Linear (mcgen_cgan_lin_dembed: dE[n] = W_lin[:, L:L+E]^T . dLinear[n]), and
//   * the discriminator's first block (mcgen_cgan_dis_window_sums + mcgen_cgan_dis_dembed).  e_n is constant over the
//     image and the 3x3 convolution pads with zeros, so the embedding's input gradient needs only, per image, the sums of
//     conv1's output gradient over the pixels where each tap reads inside the image (nine border classes), and the
//     plain sum of the 1x1 shortcut's output gradient (which the 2x2 average pool leaves equal to the block gradient's).
//
// Every reduction runs in a fixed order over fixed partitions, with no float atomics: reruns and graph replays are
// bit-identical.  Labels outside [0, M) read and write nothing (their embedding row is 0).
#include "mcgen_common.h"

namespace {
#define STREAM(s) reinterpret_cast<hipStream_t>(s)

inline int grid_for(size_t n, int block = 256, int cap = 65535) {
    size_t b = (n + block - 1) / block; if (b < 1) b = 1; if (b > (size_t)cap) b = cap; return (int)b;
}

// out[n][c], pitch Cp: z[n][c] (c < L), W[c - L][label_n] (L <= c < L + E), 0 after.
template <typename T>
__global__ __launch_bounds__(256)
void gen_input_kernel(const float* __restrict__ z, const float* __restrict__ w, const int64_t* __restrict__ label,
                      T* __restrict__ out, int N, int L, int E, int M, int Cp) {
    const size_t total = (size_t)N * Cp;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / Cp), c = (int)(i % Cp);
        float v = 0.f;
        if (c < L) {
            v = z[(size_t)n * L + c];
        } else if (c < L + E) {
            const int64_t m = label[n];
            if (m >= 0 && m < M) v = w[(size_t)(c - L) * M + m];
        }
        out[i] = Elem<T>::from_f(v);
    }
}

// out[n][p][c], pitch Cp: img[n][p][c] (c < Cimg, input pitch Cpi), W[c - Cimg][label_n] * (1 / sigma) (Cimg <= c < Cimg + E),
// 0 after.  One thread per output pixel x 8 channels.
template <typename T>
__global__ __launch_bounds__(256)
void dis_input_kernel(const T* __restrict__ img, const float* __restrict__ w, const float* __restrict__ sigma,
                      const int64_t* __restrict__ label, T* __restrict__ out, int N, int HW, int Cimg, int Cpi, int E, int M, int Cp) {
    const int cv = Cp / 8;
    const size_t total = (size_t)N * HW * cv;
    const float inv = 1.0f / sigma[0];
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i / cv;
        const int c0 = (int)(i % cv) * 8;
        const int n = (int)(pix / HW);
        const int64_t m = label[n];
        const bool ok = m >= 0 && m < M;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + j;
            float x = 0.f;
            if (c < Cimg) x = Elem<T>::to_f(img[pix * Cpi + c]);
            else if (c < Cimg + E && ok) x = w[(size_t)(c - Cimg) * M + m] * inv;
            v[j] = x;
        }
        Elem<T>::store8(out + pix * Cp + c0, v);
    }
}

// dW[e][m] (+)= sum_{n ascending, label_n == m} dE[n][e] (ld = row pitch of dE).  One thread per (e, m); the labels are
// staged through LDS 1024 at a time.
__global__ __launch_bounds__(256)
void embed_bwd_kernel(const float* __restrict__ dE, int ld, const int64_t* __restrict__ label, float* __restrict__ dW,
                      int N, int E, int M, int accumulate) {
    __shared__ int lab[1024];
    const size_t total = (size_t)E * M;
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const int e = (int)(i / M), m = (int)(i % M);
    float s = 0.f;
    for (int n0 = 0; n0 < N; n0 += 1024) {
        const int nn = min(1024, N - n0);
        __syncthreads();
        for (int k = threadIdx.x; k < nn; k += blockDim.x) {
            const int64_t l = label[n0 + k];
            lab[k] = (l >= 0 && l < M) ? (int)l : -1;
        }
        __syncthreads();
        if (i < total)
            for (int k = 0; k < nn; ++k)
                if (lab[k] == m) s += dE[(size_t)(n0 + k) * ld + e];
    }
    if (i < total) dW[i] = accumulate ? dW[i] + s : s;
}

// dE[n][e] = sum_j dlin[n][j] * W[row(j)][col0 + e], j ascending over [0, 16 C0) split into S = 1024 / E fixed slices,
// the slices added in order.  dlin is the Linear's output gradient in the engine's layout: [N, 4, 4, C0] == column
// j = p * C0 + c of output row c * 16 + p (row_perm 16, as the forward's weight image).  Grid N, 1024 threads.
template <typename T>
__global__ __launch_bounds__(1024)
void lin_dembed_kernel(const T* __restrict__ dlin, const float* __restrict__ w, float* __restrict__ dE,
                       int C0, int in_features, int col0, int E) {
    __shared__ float part[1024];
    const int n = blockIdx.x;
    const int e = threadIdx.x % E, s = threadIdx.x / E, S = 1024 / E;
    const int J = 16 * C0;
    const int per = (J + S - 1) / S;
    const int j0 = s * per, j1 = min(J, j0 + per);
    const T* d = dlin + (size_t)n * J;
    float acc = 0.f;
    for (int j = j0; j < j1; ++j) {
        const int p = j / C0, c = j % C0;
        acc += Elem<T>::to_f(d[j]) * w[(size_t)(c * 16 + p) * in_features + col0 + e];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (s == 0) {
        float t = 0.f;
        for (int k = 0; k < S; ++k) t += part[k * E + e];
        dE[(size_t)n * E + e] = t;
    }
}

// part[n][r][k][c] = sum over the columns of row r of image n in column class k (0: first column, 1: interior, 2: last)
// of dc1[n][r][col][c].  Grid (N, H), 256 threads striding the channels.
template <typename T>
__global__ __launch_bounds__(256)
void window_sums_kernel(const T* __restrict__ dc1, float* __restrict__ part, int H, int W, int C, int Cp) {
    const int n = blockIdx.x, r = blockIdx.y;
    const T* row = dc1 + ((size_t)n * H + r) * W * Cp;
    float* o = part + (((size_t)n * H + r) * 3) * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float mid = 0.f;
        for (int x = 1; x < W - 1; ++x) mid += Elem<T>::to_f(row[(size_t)x * Cp + c]);
        o[c] = Elem<T>::to_f(row[c]);
        o[C + c] = mid;
        o[2 * C + c] = Elem<T>::to_f(row[(size_t)(W - 1) * Cp + c]);
    }
}

// de[n][e] = sum_tap sum_co (W1[co][Cimg + e][tap] / s1) * S_n[tap][co] + sum_co (Wsc[co][Cimg + e] / ssc) * T_n[co]
//   S_n[(dy, dx)][co] = sum over the (row class, column class) cells where tap (dy, dx) reads inside the image of
//                       the window_sums partials (rows: first, interior rows summed ascending, last);
//   T_n[co]           = sum of dy[n][q][co] over the pooled pixels q: G = 1024 / C fixed pixel groups (q = g, g + G, ...),
//                       each summed ascending, the groups added in order.
// Grid N, 1024 threads; S and T staged in LDS (10 C floats), then S = 1024 / E fixed slices per embedding channel.
template <typename T>
__global__ __launch_bounds__(1024)
void dis_dembed_kernel(const float* __restrict__ part, const T* __restrict__ dy, const float* __restrict__ w1,
                       const float* __restrict__ wsc, const float* __restrict__ sigma1, const float* __restrict__ sigma_sc,
                       float* __restrict__ de, int H, int C, int Cin, int Cimg, int E, int HWq, int Cpq) {
    extern __shared__ float lds[];
    float* st = lds;                    // [10][C]: S per tap (dy * 3 + dx), then T
    float* red = lds + 10 * C;          // [1024]
    const int n = blockIdx.x;
    const float* pn = part + (size_t)n * H * 3 * C;
    // T partials: thread (c, g) sums the pooled pixels g, g + G, ... of channel c
    const int G = C <= 1024 ? 1024 / C : 1;
    if (threadIdx.x < G * C) {
        const int c = threadIdx.x % C, g = threadIdx.x / C;
        const T* q = dy + (size_t)n * HWq * Cpq + c;
        float t = 0.f;
        for (int i = g; i < HWq; i += G) t += Elem<T>::to_f(q[(size_t)i * Cpq]);
        red[threadIdx.x] = t;
    }
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float R[3][3];                  // [row class][column class]
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float mid = 0.f;
            for (int r = 1; r < H - 1; ++r) mid += pn[((size_t)r * 3 + k) * C + c];
            R[0][k] = pn[(size_t)k * C + c];
            R[1][k] = mid;
            R[2][k] = pn[((size_t)(H - 1) * 3 + k) * C + c];
        }
#pragma unroll
        for (int dy_ = 0; dy_ < 3; ++dy_)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                // tap dy_ reads row r + dy_ - 1: outside for the first row when dy_ == 0, for the last when dy_ == 2
                float s = 0.f;
#pragma unroll
                for (int rc = 0; rc < 3; ++rc)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) {
                        const bool in = !(dy_ == 0 && rc == 0) && !(dy_ == 2 && rc == 2) && !(dx == 0 && cc == 0) && !(dx == 2 && cc == 2);
                        if (in) s += R[rc][cc];
                    }
                st[(dy_ * 3 + dx) * C + c] = s;
            }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float t = 0.f;
        for (int g = 0; g < G; ++g) t += red[g * C + c];
        st[9 * C + c] = t;
    }
    __syncthreads();
    const int e = threadIdx.x % E, s = threadIdx.x / E, S = 1024 / E;
    const float i1 = 1.0f / sigma1[0], isc = 1.0f / sigma_sc[0];
    const int K = 10 * C;
    const int per = (K + S - 1) / S;
    const int k0 = s * per, k1 = min(K, k0 + per);
    float acc = 0.f;
    for (int k = k0; k < k1; ++k) {
        const int tap = k / C, co = k % C;
        const float wv = tap < 9 ? w1[((size_t)co * Cin + Cimg + e) * 9 + tap] * i1 : wsc[(size_t)co * Cin + Cimg + e] * isc;
        acc += wv * st[k];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (s == 0) {
        float t = 0.f;
        for (int k = 0; k < S; ++k) t += red[k * E + e];
        de[(size_t)n * E + e] = t;
    }
}

#define DISPATCH_T(dtype, F32, BF16) \
    do { if ((dtype) == MCGEN_F32) { F32; } else if ((dtype) == MCGEN_BF16) { BF16; } else return mcgen_fail("bad dtype %d", (dtype)); } while (0)
}  // namespace

extern "C" int mcgen_cgan_gen_input(const float* z, const float* w, const int64_t* label, void* out, int dtype, int N, int L,
                                    int E, int M, int Cp, void* stream) {
    MCGEN_CHECK(z && w && label && out && N > 0 && L > 0 && E > 0 && M > 0 && Cp >= L + E && Cp % 8 == 0,
                "cgan_gen_input: bad arguments (Cp >= L + E, a multiple of 8)");
    const size_t total = (size_t)N * Cp;
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(gen_input_kernel<float>, dim3(grid_for(total)), dim3(256), 0, STREAM(stream), z, w, label, (float*)out, N, L, E, M, Cp),
        hipLaunchKernelGGL(gen_input_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, STREAM(stream), z, w, label, (bf16_t*)out, N, L, E, M, Cp));
    MCGEN_LAUNCH_CHECK("cgan_gen_input"); return 0;
}

extern "C" int mcgen_cgan_dis_input(const void* img, const float* w, const float* sigma, const int64_t* label, void* out, int dtype,
                                    int N, int HW, int Cimg, int Cpi, int E, int M, int Cp, void* stream) {
    MCGEN_CHECK(img && w && sigma && label && out && N > 0 && HW > 0 && Cimg > 0 && Cpi >= Cimg && E > 0 && M > 0 &&
                Cp >= Cimg + E && Cp % 8 == 0, "cgan_dis_input: bad arguments (Cp >= Cimg + E, a multiple of 8)");
    const size_t total = (size_t)N * HW * (Cp / 8);
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(dis_input_kernel<float>, dim3(grid_for(total)), dim3(256), 0, STREAM(stream), (const float*)img, w, sigma, label, (float*)out, N, HW, Cimg, Cpi, E, M, Cp),
        hipLaunchKernelGGL(dis_input_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, STREAM(stream), (const bf16_t*)img, w, sigma, label, (bf16_t*)out, N, HW, Cimg, Cpi, E, M, Cp));
    MCGEN_LAUNCH_CHECK("cgan_dis_input"); return 0;
}

extern "C" int mcgen_cgan_embed_bwd(const float* dE, int ld, const int64_t* label, float* dW, int N, int E, int M, int accumulate,
                                    void* stream) {
    MCGEN_CHECK(dE && label && dW && N > 0 && E > 0 && M > 0 && ld >= E, "cgan_embed_bwd: bad arguments");
    const size_t total = (size_t)E * M;
    hipLaunchKernelGGL(embed_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, STREAM(stream), dE, ld, label, dW, N, E, M, accumulate);
    MCGEN_LAUNCH_CHECK("cgan_embed_bwd"); return 0;
}

extern "C" int mcgen_cgan_lin_dembed(const void* dlin, const float* w, float* dE, int dtype, int N, int C0, int in_features, int col0,
                                     int E, void* stream) {
    MCGEN_CHECK(dlin && w && dE && N > 0 && C0 > 0 && E > 0 && E <= 256 && 256 % E == 0 && col0 >= 0 && col0 + E <= in_features,
                "cgan_lin_dembed: bad arguments (E must divide 256, col0 + E <= in_features)");
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(lin_dembed_kernel<float>, dim3(N), dim3(1024), 0, STREAM(stream), (const float*)dlin, w, dE, C0, in_features, col0, E),
        hipLaunchKernelGGL(lin_dembed_kernel<bf16_t>, dim3(N), dim3(1024), 0, STREAM(stream), (const bf16_t*)dlin, w, dE, C0, in_features, col0, E));
    MCGEN_LAUNCH_CHECK("cgan_lin_dembed"); return 0;
}

extern "C" int mcgen_cgan_dis_window_sums(const void* dc1, float* part, int dtype, int N, int H, int W, int C, int Cp, void* stream) {
    MCGEN_CHECK(dc1 && part && N > 0 && H >= 2 && W >= 2 && C > 0 && Cp >= C && H <= 65535,
                "cgan_dis_window_sums: bad arguments (maps of at least 2 x 2)");
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(window_sums_kernel<float>, dim3(N, H), dim3(256), 0, STREAM(stream), (const float*)dc1, part, H, W, C, Cp),
        hipLaunchKernelGGL(window_sums_kernel<bf16_t>, dim3(N, H), dim3(256), 0, STREAM(stream), (const bf16_t*)dc1, part, H, W, C, Cp));
    MCGEN_LAUNCH_CHECK("cgan_dis_window_sums"); return 0;
}

extern "C" int mcgen_cgan_dis_dembed(const float* part, const void* dy, const float* w1, const float* wsc, const float* sigma1,
                                     const float* sigma_sc, float* de, int dtype, int N, int H, int C, int Cin, int Cimg, int E,
                                     int HWq, int Cpq, void* stream) {
    MCGEN_CHECK(part && dy && w1 && wsc && sigma1 && sigma_sc && de && N > 0 && H >= 2 && C > 0 && Cpq >= C && HWq > 0 &&
                E > 0 && E <= 256 && 256 % E == 0 && Cimg >= 0 && Cimg + E <= Cin,
                "cgan_dis_dembed: bad arguments (E must divide 256, Cimg + E <= Cin)");
    const size_t lds = (size_t)(10 * C + 1024) * sizeof(float);
    MCGEN_CHECK(C <= 1024 && lds <= 64 * 1024, "cgan_dis_dembed: %d channels do not fit the LDS plan (at most 1024)", C);
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(dis_dembed_kernel<float>, dim3(N), dim3(1024), lds, STREAM(stream), part, (const float*)dy, w1, wsc, sigma1, sigma_sc, de, H, C, Cin, Cimg, E, HWq, Cpq),
        hipLaunchKernelGGL(dis_dembed_kernel<bf16_t>, dim3(N), dim3(1024), lds, STREAM(stream), part, (const bf16_t*)dy, w1, wsc, sigma1, sigma_sc, de, H, C, Cin, Cimg, E, HWq, Cpq));
    MCGEN_LAUNCH_CHECK("cgan_dis_dembed"); return 0;
}
