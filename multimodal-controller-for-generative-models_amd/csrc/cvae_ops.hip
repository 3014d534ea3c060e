// CVAE label-embedding kernels (gfx950): the two places where the reference's CVAE (src/models/cvae.py) differs from MCVAE
// once the MultimodalControllers are gone.
//
//   Encoder: x = cat((img + 1) / 2, embedding(one_hot(label)) broadcast over H x W) -> Conv2d(C + E, h0, 4, 2, 1)  (cvae.py:58-63)
//   Decoder: x = cat(z, embedding(one_hot(label)))                                  -> Linear(L + E, features)      (cvae.py:92-96)
//   embedding(one_hot(label)) = W[:, label], W = embedding.weight [E, M]
//
// Forward: mcgen_cvae_enc_input writes the encoder's NHWC input with the embedding channels appended, straight from the NCHW
// image; mcgen_cvae_latent_fwd turns the mu | logvar head output into mu, logvar, the decoder Linear's input row
// [z (+) W[:, label] (+) 0] and the KL term.  Backward: mcgen_cvae_latent_bwd packs [dmu | dlogvar | 0] from the Linear's input
// gradient and hands out its embedding columns; mcgen_cvae_enc_dembed gives the encoder embedding's input gradient without the
// first convolution's input gradient: e_n is constant over the image and the convolution pads with zeros, so
//   dE[n][e] = sum_{kh, kw} sum_co W[co][C + e][kh][kw] * S_n[kh][kw][co],
// S_n[kh][kw] = the sum of the convolution's output gradient over the output pixels where tap (kh, kw) reads inside the image.
// For kernel 4, stride 2, padding 1 on an even-sized image tap 0 misses the first output row / column only, tap 3 the last
// only, taps 1 and 2 none: the per-row first / interior / last column sums of mcgen_cgan_dis_window_sums are enough.
// The table gradient dW[:, m] = sum_{label_n == m} dE[n] is mcgen_cgan_embed_bwd.
//
// Every reduction runs in a fixed order over fixed partitions, with no float atomics: reruns and graph replays are
// bit-identical.  Labels outside [0, M) read a zero embedding row and write nothing.
#include "mcgen_common.h"

namespace {
#define STREAM(s) reinterpret_cast<hipStream_t>(s)

// out[n][p][c], pitch Cp: (img[n][c][p] + 1) / 2 (c < C), W[c - C][label_n] (C <= c < C + E), 0 after.  Grid (N, Y): the
// workgroup stages its image's embedding row in LDS once, then each thread writes 8 channels of a pixel with one 16-byte
// (bf16) or two 16-byte (fp32) stores.
template <typename T>
__global__ __launch_bounds__(256)
void enc_input_kernel(const float* __restrict__ img, const float* __restrict__ w, const int64_t* __restrict__ label,
                      T* __restrict__ out, int HW, int C, int E, int M, int Cp) {
    extern __shared__ float emb[];      // [E]
    const int n = blockIdx.x;
    const int64_t m = label[n];
    const bool ok = m >= 0 && m < M;
    for (int e = threadIdx.x; e < E; e += blockDim.x) emb[e] = ok ? w[(size_t)e * M + m] : 0.f;
    __syncthreads();
    const int cv = Cp / 8;
    const int total = HW * cv;
    const float* im = img + (size_t)n * C * HW;
    T* o = out + (size_t)n * HW * Cp;
    for (int i = blockIdx.y * blockDim.x + threadIdx.x; i < total; i += gridDim.y * blockDim.x) {
        const int p = i / cv, c0 = (i % cv) * 8;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + j;
            float x = 0.f;
            if (c < C) x = (im[(size_t)c * HW + p] + 1.0f) * 0.5f;
            else if (c < C + E) x = emb[c - C];
            v[j] = x;
        }
        Elem<T>::store8(o + (size_t)p * Cp + c0, v);
    }
}

// de[n][e] = sum_tap sum_co W[co][Cimg + e][tap] * S_n[tap][co], tap = kh * 4 + kw.
//   S_n[(kh, kw)][co] = sum over the (row class, column class) cells where the tap reads inside the image of the window_sums
//                       partials part[n][r][k][co] (rows: first, interior rows summed ascending, last).
// Grid N, 1024 threads; S staged in LDS (16 C floats), then S = 1024 / E fixed slices of the (tap, co) range per embedding
// channel, the slices added in order.
__global__ __launch_bounds__(1024)
void enc_dembed_kernel(const float* __restrict__ part, const float* __restrict__ w, float* __restrict__ de,
                       int H, int C, int Cin, int Cimg, int E) {
    extern __shared__ float lds[];
    float* st = lds;                    // [16][C]
    float* red = lds + 16 * C;          // [1024]
    const int n = blockIdx.x;
    const float* pn = part + (size_t)n * H * 3 * C;
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
        for (int kh = 0; kh < 4; ++kh)
#pragma unroll
            for (int kw = 0; kw < 4; ++kw) {
                // tap kh reads input row 2 r + kh - 1: outside for the first output row when kh == 0, the last when kh == 3
                float s = 0.f;
#pragma unroll
                for (int rc = 0; rc < 3; ++rc)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) {
                        const bool in = !(kh == 0 && rc == 0) && !(kh == 3 && rc == 2) && !(kw == 0 && cc == 0) && !(kw == 3 && cc == 2);
                        if (in) s += R[rc][cc];
                    }
                st[(kh * 4 + kw) * C + c] = s;
            }
    }
    __syncthreads();
    const int e = threadIdx.x % E, s = threadIdx.x / E, S = 1024 / E;
    const int K = 16 * C;
    const int per = (K + S - 1) / S;
    const int k0 = s * per, k1 = min(K, k0 + per);
    float acc = 0.f;
    for (int k = k0; k < k1; ++k) {
        const int tap = k / C, co = k % C;
        acc += w[((size_t)co * Cin + Cimg + e) * 16 + tap] * st[k];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (s == 0) {
        float t = 0.f;
        for (int k = 0; k < S; ++k) t += red[k * E + e];
        de[(size_t)n * E + e] = t;
    }
}

// One workgroup per sample.  ml[n] (pitch ldm) = [mu (L) | logvar (L)] in the compute dtype:
//   mu / logvar [N][L] fp32;  zrow[n] (pitch Cp) = [z (L) | W[:, label_n] (E) | 0],  z = mu + eps * exp(logvar / 2) (eps given)
//   or mu;  kl[n] = 0.5 * sum_j (mu^2 + exp(logvar) - 1 - logvar): thread t sums columns t, t + 256, ... ascending, then a
//   fixed binary tree over the 256 partials.
template <typename T>
__global__ __launch_bounds__(256)
void latent_fwd_kernel(const T* __restrict__ ml, int ldm, const float* __restrict__ eps, const float* __restrict__ w,
                       const int64_t* __restrict__ label, float* __restrict__ mu, float* __restrict__ logvar,
                       T* __restrict__ zrow, float* __restrict__ kl, int L, int E, int M, int Cp) {
    __shared__ float red[256];
    const int n = blockIdx.x;
    const T* row = ml + (size_t)n * ldm;
    T* zr = zrow + (size_t)n * Cp;
    float acc = 0.f;
    for (int j = threadIdx.x; j < L; j += blockDim.x) {
        const float m_ = Elem<T>::to_f(row[j]), lv = Elem<T>::to_f(row[L + j]);
        mu[(size_t)n * L + j] = m_;
        logvar[(size_t)n * L + j] = lv;
        const float z = eps ? m_ + eps[(size_t)n * L + j] * expf(0.5f * lv) : m_;
        zr[j] = Elem<T>::from_f(z);
        acc += m_ * m_ + expf(lv) - 1.0f - lv;
    }
    const int64_t m = label[n];
    const bool ok = m >= 0 && m < M;
    for (int c = L + threadIdx.x; c < Cp; c += blockDim.x)
        zr[c] = Elem<T>::from_f((c < L + E && ok) ? w[(size_t)(c - L) * M + m] : 0.f);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) kl[n] = 0.5f * red[0];
}

// kld[0] = sum_n kl[n], n ascending.
__global__ void kl_total_kernel(const float* __restrict__ kl, float* __restrict__ kld, int N) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float t = 0.f;
        for (int n = 0; n < N; ++n) t += kl[n];
        kld[0] = t;
    }
}

// dml[n] (pitch Cq) = [dmu (L) | dlogvar (L) | 0] in the compute dtype from dz = dzrow[n][0 .. L) (pitch ldz):
//   dmu = dz + mu * inv_numel;  dlogvar = dz * eps * 0.5 * exp(logvar / 2) + 0.5 * (exp(logvar) - 1) * inv_numel;
// de[n][e] (optional, fp32) = dzrow[n][L + e].  One thread per output element.
template <typename T>
__global__ __launch_bounds__(256)
void latent_bwd_kernel(const T* __restrict__ dzrow, int ldz, const float* __restrict__ mu, const float* __restrict__ logvar,
                       const float* __restrict__ eps, float inv_numel, T* __restrict__ dml, float* __restrict__ de,
                       int N, int L, int E, int Cq) {
    const int W = Cq + E;
    const size_t total = (size_t)N * W;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int n = (int)(i / W), c = (int)(i % W);
        const T* dz = dzrow + (size_t)n * ldz;
        if (c >= Cq) {
            if (de) de[(size_t)n * E + (c - Cq)] = Elem<T>::to_f(dz[L + c - Cq]);
            continue;
        }
        float v = 0.f;
        if (c < L) {
            v = Elem<T>::to_f(dz[c]) + mu[(size_t)n * L + c] * inv_numel;
        } else if (c < 2 * L) {
            const int j = c - L;
            const float lv = logvar[(size_t)n * L + j];
            v = Elem<T>::to_f(dz[j]) * eps[(size_t)n * L + j] * 0.5f * expf(0.5f * lv) + 0.5f * (expf(lv) - 1.0f) * inv_numel;
        }
        dml[(size_t)n * Cq + c] = Elem<T>::from_f(v);
    }
}

inline int grid_for(size_t n, int block = 256, int cap = 65535) {
    size_t b = (n + block - 1) / block; if (b < 1) b = 1; if (b > (size_t)cap) b = cap; return (int)b;
}

#define DISPATCH_T(dtype, F32, BF16) \
    do { if ((dtype) == MCGEN_F32) { F32; } else if ((dtype) == MCGEN_BF16) { BF16; } else return mcgen_fail("bad dtype %d", (dtype)); } while (0)
}  // namespace

extern "C" int mcgen_cvae_enc_input(const float* img, const float* w, const int64_t* label, void* out, int dtype, int N, int HW,
                                    int C, int E, int M, int Cp, void* stream) {
    MCGEN_CHECK(img && w && label && out && N > 0 && HW > 0 && C > 0 && E > 0 && E <= 4096 && M > 0 && Cp >= C + E && Cp % 8 == 0,
                "cvae_enc_input: bad arguments (Cp >= C + E, a multiple of 8; E <= 4096)");
    MCGEN_CHECK(dtype == MCGEN_F32 || dtype == MCGEN_BF16, "cvae_enc_input: bad dtype %d", dtype);
    const size_t per_image = (size_t)HW * (Cp / 8);
    MCGEN_CHECK(per_image <= (size_t)1 << 30, "cvae_enc_input: image of %d pixels x %d channels is too large", HW, Cp);
    const dim3 grid(N, grid_for(per_image, 256, 8));
    const size_t lds = (size_t)E * sizeof(float);
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(enc_input_kernel<float>, grid, dim3(256), lds, STREAM(stream), img, w, label, (float*)out, HW, C, E, M, Cp),
        hipLaunchKernelGGL(enc_input_kernel<bf16_t>, grid, dim3(256), lds, STREAM(stream), img, w, label, (bf16_t*)out, HW, C, E, M, Cp));
    MCGEN_LAUNCH_CHECK("cvae_enc_input"); return 0;
}

extern "C" int mcgen_cvae_enc_dembed(const float* part, const float* w, float* de, int N, int H, int C, int Cin, int Cimg, int E,
                                     void* stream) {
    MCGEN_CHECK(part && w && de && N > 0 && H >= 2 && C > 0 && E > 0 && E <= 256 && 256 % E == 0 && Cimg >= 0 && Cimg + E <= Cin,
                "cvae_enc_dembed: bad arguments (E must divide 256, Cimg + E <= Cin, output maps of at least 2 rows)");
    const size_t lds = (size_t)(16 * C + 1024) * sizeof(float);
    MCGEN_CHECK(lds <= 64 * 1024, "cvae_enc_dembed: %d channels do not fit the LDS plan (at most 960)", C);
    hipLaunchKernelGGL(enc_dembed_kernel, dim3(N), dim3(1024), lds, STREAM(stream), part, w, de, H, C, Cin, Cimg, E);
    MCGEN_LAUNCH_CHECK("cvae_enc_dembed"); return 0;
}

extern "C" int mcgen_cvae_latent_fwd(const void* ml, int ldm, const float* eps, const float* w, const int64_t* label, float* mu,
                                     float* logvar, void* zrow, float* kl, float* kld, int dtype, int N, int L, int E, int M, int Cp,
                                     void* stream) {
    MCGEN_CHECK(ml && w && label && mu && logvar && zrow && kl && kld && N > 0 && L > 0 && E > 0 && M > 0 && ldm >= 2 * L &&
                Cp >= L + E && Cp % 8 == 0, "cvae_latent_fwd: bad arguments (ldm >= 2 L; Cp >= L + E, a multiple of 8)");
    MCGEN_CHECK(dtype == MCGEN_F32 || dtype == MCGEN_BF16, "cvae_latent_fwd: bad dtype %d", dtype);
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(latent_fwd_kernel<float>, dim3(N), dim3(256), 0, STREAM(stream), (const float*)ml, ldm, eps, w, label, mu, logvar, (float*)zrow, kl, L, E, M, Cp),
        hipLaunchKernelGGL(latent_fwd_kernel<bf16_t>, dim3(N), dim3(256), 0, STREAM(stream), (const bf16_t*)ml, ldm, eps, w, label, mu, logvar, (bf16_t*)zrow, kl, L, E, M, Cp));
    MCGEN_LAUNCH_CHECK("cvae_latent_fwd");
    hipLaunchKernelGGL(kl_total_kernel, dim3(1), dim3(64), 0, STREAM(stream), kl, kld, N);
    MCGEN_LAUNCH_CHECK("cvae_latent_fwd"); return 0;
}

extern "C" int mcgen_cvae_latent_bwd(const void* dzrow, int ldz, const float* mu, const float* logvar, const float* eps,
                                     float inv_numel, void* dml, float* de, int dtype, int N, int L, int E, int Cq, void* stream) {
    MCGEN_CHECK(dzrow && mu && logvar && eps && dml && N > 0 && L > 0 && E >= 0 && ldz >= L + E && Cq >= 2 * L && Cq % 8 == 0 &&
                (de || E == 0), "cvae_latent_bwd: bad arguments (ldz >= L + E; Cq >= 2 L, a multiple of 8; de with E > 0)");
    MCGEN_CHECK(dtype == MCGEN_F32 || dtype == MCGEN_BF16, "cvae_latent_bwd: bad dtype %d", dtype);
    const size_t total = (size_t)N * (Cq + E);
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(latent_bwd_kernel<float>, dim3(grid_for(total)), dim3(256), 0, STREAM(stream), (const float*)dzrow, ldz, mu, logvar, eps, inv_numel, (float*)dml, de, N, L, E, Cq),
        hipLaunchKernelGGL(latent_bwd_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, STREAM(stream), (const bf16_t*)dzrow, ldz, mu, logvar, eps, inv_numel, (bf16_t*)dml, de, N, L, E, Cq));
    MCGEN_LAUNCH_CHECK("cvae_latent_bwd"); return 0;
}
