// Incremental eval-mode ancestral sampling of MCGatedPixelCNN (gfx950): every pixel of every layer is computed once.
// Reference: models/mcpixelcnn.py:47-61 (the two stacks), :89-112 (head, generate); the crop of the padded stacks follows
// pixelcnn_engine.py.  In eval mode BatchNorm is a per-channel affine and every MultimodalController row belongs to one
// sample, so samples are independent and a workgroup owns a tile of samples for every layer:
//   row launch (row i):     all layers' vertical stacks, gate_v and vert_to_horiz for the W pixels of row i;
//   column launch (i, j):   all layers' horizontal path, the head, the softmax and the draw for pixel (i, j).
// Every product is an MFMA GEMM tile: rows = (sample, pixel) of the tile, columns = output channels, A fragments from
// LDS (or gathered from the embedding table), B fragments streamed from the packed weights ([Nout][Kp], K contiguous).
// bf16: v_mfma_f32_16x16x32_bf16; fp32: v_mfma_f32_16x16x4_f32 (exact f32).  Activations are rounded to the compute
// dtype where PixelCNNEngine.forward stores them; vert_to_horiz stays fp32 (the engine adds it inside one conv).
#include "mcgen_common.h"

namespace {
#define STREAM(s) reinterpret_cast<hipStream_t>(s)
constexpr int PX_THREADS = 256, PX_WAVES = PX_THREADS / 64;
constexpr int PX_ROWS = 32;                 // target GEMM rows (samples x pixels) of a row-launch workgroup
constexpr int PX_LDS_MAX = 160 * 1024;

__host__ __device__ inline int r16(int x) { return (x + 15) / 16 * 16; }
__host__ __device__ inline int r32(int x) { return (x + 31) / 32 * 32; }
__host__ __device__ inline size_t a16(size_t x) { return (x + 15) / 16 * 16; }

// ---- packed parameter layout (pixelcnn_sampler.py builds the same) -------------------------------------------------
// weights, per layer: Wv [2C][r32(KV)], Wv2h [2C][r32(2C)], Wh [2C][r32(KH)], Wr [r16(C)][r32(C)] with KV = 21C / 6C,
// KH = 3C / 2C for layer 0 / the others; then the head W0 [r16(Hd)][r32(C)], W4 [r16(Kq)][r32(Hd)].
// fp32, per layer (13C): bv, bv2h, bh [2C each], br, scv, shv, sch, shh, scr, shr [C each]; head b0, sc0, sh0 [Hd], b4 [Kq].
// MC code rows: [L][3 (gate_v, gate_h, horiz_resid)][N][C], then the head's [N][Hd].
struct Geo {
    int C, L, Hd, Kq;
    __device__ __host__ int kv(int l) const { return (l == 0 ? 21 : 6) * C; }
    __device__ __host__ int kh(int l) const { return (l == 0 ? 3 : 2) * C; }
    __device__ __host__ size_t layer_elems(int l) const {
        return (size_t)2 * C * (r32(kv(l)) + r32(2 * C) + r32(kh(l))) + (size_t)r16(C) * r32(C);
    }
    __device__ __host__ size_t layer_off(int l) const { return l == 0 ? 0 : layer_elems(0) + (size_t)(l - 1) * layer_elems(1); }
    __device__ __host__ size_t wv(int l) const { return layer_off(l); }
    __device__ __host__ size_t wv2h(int l) const { return wv(l) + (size_t)2 * C * r32(kv(l)); }
    __device__ __host__ size_t wh(int l) const { return wv2h(l) + (size_t)2 * C * r32(2 * C); }
    __device__ __host__ size_t wr(int l) const { return wh(l) + (size_t)2 * C * r32(kh(l)); }
    __device__ __host__ size_t w0() const { return layer_off(L); }
    __device__ __host__ size_t w4() const { return w0() + (size_t)r16(Hd) * r32(C); }
    __device__ __host__ size_t p(int l) const { return (size_t)l * 13 * C; }
};

// ---- MFMA fragments ---------------------------------------------------------------------------------------------------
template <typename T> struct Frag;
template <> struct Frag<bf16_t> {
    typedef bf16x8 v; static constexpr int VL = 8;
    static __device__ __forceinline__ v zero() { v z; for (int i = 0; i < 8; ++i) z[i] = (bf16_t)0.f; return z; }
    static __device__ __forceinline__ f32x4 mma(const v& a, const v& b, f32x4 acc) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
};
template <> struct Frag<float> {
    // four k values per lane; MFMA step s takes element s of A and B, so both walk k in the same permuted order
    typedef f32x4 v; static constexpr int VL = 4;
    static __device__ __forceinline__ v zero() { v z = {0.f, 0.f, 0.f, 0.f}; return z; }
    static __device__ __forceinline__ f32x4 mma(const v& a, const v& b, f32x4 acc) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
        return acc;
    }
};

// out[m][col] = sum_k A(m, k) B[col][k] for m < M, col < Nout (a multiple of 16), k < Kp (a multiple of 32).
// Wave w owns the 16-column tiles w, w + 4, ...; two 16-row tiles share every B fragment; U B fragments per lane are in
// flight before their MFMAs.  afrag(m, k) returns the VL elements A[m][k .. k + VL) (zero outside the operand).
template <typename T, typename AF, typename EF>
__device__ __forceinline__ void gemm(int M, int Nout, int Kp, const T* __restrict__ B, AF afrag, EF epi) {
    typedef Frag<T> F;
    typedef typename F::v V;
    constexpr int VL = F::VL, KS = 4 * VL, U = 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lk = (lane >> 4) * VL;
    const int mtiles = (M + 15) / 16, ntiles = Nout / 16;
    for (int mt0 = 0; mt0 < mtiles; mt0 += 2) {
        const bool two = mt0 + 1 < mtiles;
        for (int nt = wave; nt < ntiles; nt += PX_WAVES) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
            const T* b = B + (size_t)(nt * 16 + lr) * Kp + lk;
            for (int k0 = 0; k0 < Kp; k0 += KS * U) {
                V bf[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    bf[u] = k0 + u * KS < Kp ? *reinterpret_cast<const V*>(b + k0 + u * KS) : F::zero();
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = k0 + u * KS;
                    if (k >= Kp) break;
                    acc0 = F::mma(afrag(mt0 * 16 + lr, k + lk), bf[u], acc0);
                    if (two) acc1 = F::mma(afrag(mt0 * 16 + 16 + lr, k + lk), bf[u], acc1);
                }
            }
            const int col = nt * 16 + lr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mt0 * 16 + (lane >> 4) * 4 + r;
                if (m < M) epi(m, col, acc0[r]);
                if (two && m + 16 < M) epi(m + 16, col, acc1[r]);
            }
        }
    }
}

template <typename T>
__device__ __forceinline__ typename Frag<T>::v ldfrag(const T* p) { return *reinterpret_cast<const typename Frag<T>::v*>(p); }
template <typename T> __device__ __forceinline__ T rnd(float x) { return (T)x; }
template <typename T> __device__ __forceinline__ float f(T x) { return (float)x; }

__device__ __forceinline__ int clamp_code(int64_t v, int Kq) { return v < 0 ? 0 : (v >= Kq ? Kq - 1 : (int)v); }

// gated activation (pixelcnn_ops.hip gated_fwd_body): code * relu(a * sc + sh) * sigmoid(b)
__device__ __forceinline__ float gate(float a, float b, float sc, float sh, float code) {
    return code * fmaxf(fmaf(a, sc, sh), 0.f) / (1.f + expf(-b));
}

// ---- row launch -------------------------------------------------------------------------------------------------------
struct RowLds {
    int SR, M, ldh;
    size_t cd, xv, hv, bytes;
    __host__ __device__ RowLds(int W, int C, int esz) {
        SR = W >= PX_ROWS ? 1 : PX_ROWS / W;
        M = SR * W;
        ldh = 2 * C + 16 / esz;
        cd = 0;
        xv = a16((size_t)SR * 3 * (W + 6) * 4);
        hv = xv + a16((size_t)SR * 2 * (W + 2) * C * esz);
        bytes = hv + (size_t)r16(M) * ldh * esz;
    }
};

// COND: ConditionalGatedPixelCNN (models/cpixelcnn.py): P.mc holds per-sample rows [L][N][2C] added to both gate inputs, and
// nothing is multiplied by a controller row
template <typename T, bool COND = false>
__global__ __launch_bounds__(PX_THREADS) void px_row_kernel(const mcgen_px_sample_t P, int i) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int C = P.C, C2 = 2 * C, W = P.W, H = P.H, N = P.N, L = P.L;
    const Geo g{C, L, P.Hd, P.Kq};
    const RowLds lay(W, C, sizeof(T));
    const int SR = lay.SR, M = lay.M, ldh = lay.ldh, n0 = blockIdx.x * SR, W2 = W + 2, W6 = W + 6;
    int* cd = reinterpret_cast<int*>(smem + lay.cd);       // [SR][3][W + 6] codes of rows i-3 .. i-1, -1 = zero padding
    T* xv = reinterpret_cast<T*>(smem + lay.xv);           // [SR][2][W + 2][C] out_v of the layer below, rows i-1 and i
    T* hv = reinterpret_cast<T*>(smem + lay.hv);           // [M][ldh] h_vert (pre-gate) of this layer
    const T* emb = reinterpret_cast<const T*>(P.emb);
    const T* wts = reinterpret_cast<const T*>(P.w);
    T* ov = reinterpret_cast<T*>(P.ov);
    const int tid = threadIdx.x;
    for (int e = tid; e < SR * 3 * W6; e += PX_THREADS) {
        const int cc = e % W6, dr = (e / W6) % 3, s = e / (3 * W6);
        const int n = n0 + s, r = i - 3 + dr, col = cc - 3;
        cd[e] = (n < N && r >= 0 && col >= 0 && col < W) ? clamp_code(P.codes[((size_t)n * H + r) * W + col], P.Kq) : -1;
    }
    for (int e = tid; e < SR * 2 * W2 * C; e += PX_THREADS) xv[e] = rnd<T>(0.f);
    __syncthreads();
    typedef typename Frag<T>::v V;
    for (int l = 0; l < L; ++l) {
        const float* pp = P.p + g.p(l);
        const float *bv = pp, *bv2h = pp + C2;
        const int KV = g.kv(l);
        auto epi_hv = [&](int m, int col, float a) { hv[(size_t)m * ldh + col] = rnd<T>(a + bv[col]); };
        if (l == 0) {
            // the 4x7 mask-A stack: its live taps (dr < 3) read rows i-3 .. i-1, columns j-3 .. j+3 of the embedded codes
            gemm<T>(M, C2, r32(KV), wts + g.wv(0), [&](int m, int k) -> V {
                if (m >= M || k >= KV) return Frag<T>::zero();
                const int s = m / W, j = m % W, tap = k / C, c = k % C;
                const int code = cd[(s * 3 + tap / 7) * W6 + j + tap % 7];
                return code < 0 ? Frag<T>::zero() : ldfrag<T>(emb + (size_t)code * C + c);
            }, epi_hv);
        } else {
            // the 2x3 stack: rows i-1, i and columns j-1 .. j+1 of out_v of layer l-1
            gemm<T>(M, C2, r32(KV), wts + g.wv(l), [&](int m, int k) -> V {
                if (m >= M || k >= KV) return Frag<T>::zero();
                const int s = m / W, j = m % W, tap = k / C, c = k % C;
                return ldfrag<T>(xv + ((size_t)(s * 2 + tap / 3) * W2 + j + tap % 3) * C + c);
            }, epi_hv);
        }
        __syncthreads();
        // vert_to_horiz on the pre-gate h_vert (mcpixelcnn.py:55), kept in fp32 for the column launches
        gemm<T>(M, C2, r32(C2), wts + g.wv2h(l), [&](int m, int k) -> V {
            return (m >= M || k >= C2) ? Frag<T>::zero() : ldfrag<T>(hv + (size_t)m * ldh + k);
        }, [&](int m, int col, float a) {
            const int n = n0 + m / W;
            if (n < N) P.v2h[(((size_t)l * N + n) * W + m % W) * C2 + col] = a + bv2h[col];
        });
        if (l + 1 < L) {
            // gate_v -> out_v of row i (LDS row slot 1 for the next layer, and the global ring for row i + 1); the next
            // layer's row i-1 comes from the ring slot the previous row launch wrote
            const float *scv = pp + 7 * C, *shv = pp + 8 * C;
            const float* code_v = P.mc + (size_t)(l * 3) * N * C;
            const int par = i & 1;
            for (int e = tid; e < M * C; e += PX_THREADS) {
                const int c = e % C, m = e / C, s = m / W, j = m % W, n = n0 + s;
                float o = 0.f, prev = 0.f;
                if (n < N) {
                    if (COND) {
                        const float* row = P.mc + ((size_t)l * N + n) * C2;
                        o = gate(f(hv[(size_t)m * ldh + c]) + row[c], f(hv[(size_t)m * ldh + C + c]) + row[C + c], scv[c], shv[c], 1.f);
                    } else {
                        o = gate(f(hv[(size_t)m * ldh + c]), f(hv[(size_t)m * ldh + C + c]), scv[c], shv[c], code_v[(size_t)n * C + c]);
                    }
                    const T ot = rnd<T>(o);
                    ov[((((size_t)l * N + n) * 2 + par) * W + j) * C + c] = ot;
                    o = f(ot);
                    if (i > 0) prev = f(ov[((((size_t)l * N + n) * 2 + (par ^ 1)) * W + j) * C + c]);
                }
                xv[((size_t)(s * 2 + 1) * W2 + j + 1) * C + c] = rnd<T>(o);
                xv[((size_t)(s * 2) * W2 + j + 1) * C + c] = rnd<T>(prev);
            }
        }
        __syncthreads();
    }
}

// ---- column launch ----------------------------------------------------------------------------------------------------
struct ColLds {
    int lda, lds_, ldo, ldz;
    size_t xa, s, oh, xc, z, lg, bytes;
    __host__ __device__ ColLds(int C, int Hd, int Kq, int esz) {
        const int pad = 16 / esz;
        lda = 3 * C + pad; lds_ = 2 * C + pad; ldo = C + pad; ldz = Hd + pad;
        xa = 0;
        s = a16((size_t)16 * lda * esz);
        oh = s + a16((size_t)16 * lds_ * esz);
        xc = oh + a16((size_t)16 * ldo * esz);
        z = xc + a16((size_t)16 * C * esz);
        lg = z + a16((size_t)16 * ldz * esz);
        bytes = lg + (size_t)16 * Kq * 4;
    }
};

template <typename T, bool COND = false>
__global__ __launch_bounds__(PX_THREADS) void px_col_kernel(const mcgen_px_sample_t P, int i, int j) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int C = P.C, C2 = 2 * C, W = P.W, H = P.H, N = P.N, L = P.L, Hd = P.Hd, Kq = P.Kq;
    const Geo g{C, L, Hd, Kq};
    const ColLds lay(C, Hd, Kq, sizeof(T));
    T* xa = reinterpret_cast<T*>(smem + lay.xa);           // [16][lda] horizontal-stack taps of this layer
    T* sv = reinterpret_cast<T*>(smem + lay.s);            // [16][2C] s = vert_to_horiz + horiz_stack
    T* oh = reinterpret_cast<T*>(smem + lay.oh);           // [16][C] out_h
    T* xc = reinterpret_cast<T*>(smem + lay.xc);           // [16][C] x_h of the current layer at (i, j)
    T* zz = reinterpret_cast<T*>(smem + lay.z);            // [16][Hd] head activation, the last 1x1's operand
    float* lg = reinterpret_cast<float*>(smem + lay.lg);   // [16][Kq] logits
    const T* emb = reinterpret_cast<const T*>(P.emb);
    const T* wts = reinterpret_cast<const T*>(P.w);
    T* xh = reinterpret_cast<T*>(P.xh);
    const int tid = threadIdx.x, n0 = blockIdx.x * 16, M = 16;
    typedef typename Frag<T>::v V;
    for (int l = 0; l < L; ++l) {
        const float* pp = P.p + g.p(l);
        const float *bh = pp + 4 * C, *br = pp + 6 * C, *sch = pp + 9 * C, *shh = pp + 10 * C, *scr = pp + 11 * C, *shr = pp + 12 * C;
        const float* code_h = P.mc + (size_t)(l * 3 + 1) * N * C;
        const float* code_r = P.mc + (size_t)(l * 3 + 2) * N * C;
        const int KH = g.kh(l);
        if (l == 0) {
            // the 1x4 mask-A stack: live taps read columns j-3 .. j-1 of row i of the embedded codes
            for (int e = tid; e < 16 * 3 * C; e += PX_THREADS) {
                const int c = e % C, dc = (e / C) % 3, m = e / (3 * C), n = n0 + m, col = j - 3 + dc;
                T v = rnd<T>(0.f);
                if (n < N && col >= 0) v = emb[(size_t)clamp_code(P.codes[((size_t)n * H + i) * W + col], Kq) * C + c];
                xa[(size_t)m * lay.lda + dc * C + c] = v;
            }
        } else {
            // the 1x2 stack: x_h of layer l-1 at columns j-1 (written by the previous column launch) and j (in LDS)
            for (int e = tid; e < 16 * C; e += PX_THREADS) {
                const int c = e % C, m = e / C, n = n0 + m;
                T v = rnd<T>(0.f);
                if (n < N && j > 0) v = xh[(((size_t)(l - 1) * N + n) * W + j - 1) * C + c];
                xa[(size_t)m * lay.lda + c] = v;
                xa[(size_t)m * lay.lda + C + c] = xc[(size_t)m * C + c];
            }
        }
        __syncthreads();
        gemm<T>(M, C2, r32(KH), wts + g.wh(l), [&](int m, int k) -> V {
            return k >= KH ? Frag<T>::zero() : ldfrag<T>(xa + (size_t)m * lay.lda + k);
        }, [&](int m, int col, float a) {
            const int n = n0 + m;
            const float v2h = n < N ? P.v2h[(((size_t)l * N + n) * W + j) * C2 + col] : 0.f;
            sv[(size_t)m * lay.lds_ + col] = rnd<T>(a + bh[col] + v2h);
        });
        __syncthreads();
        for (int e = tid; e < 16 * C; e += PX_THREADS) {
            const int c = e % C, m = e / C, n = n0 + m;
            float o = 0.f;
            if (n < N) {
                if (COND) {
                    const float* row = P.mc + ((size_t)l * N + n) * C2;
                    o = gate(f(sv[(size_t)m * lay.lds_ + c]) + row[c], f(sv[(size_t)m * lay.lds_ + C + c]) + row[C + c], sch[c], shh[c], 1.f);
                } else {
                    o = gate(f(sv[(size_t)m * lay.lds_ + c]), f(sv[(size_t)m * lay.lds_ + C + c]), sch[c], shh[c], code_h[(size_t)n * C + c]);
                }
            }
            oh[(size_t)m * lay.ldo + c] = rnd<T>(o);
        }
        __syncthreads();
        // horiz_resid: 1x1 -> BN -> MC, + x_h (mcpixelcnn.py:57-60)
        gemm<T>(M, r16(C), r32(C), wts + g.wr(l), [&](int m, int k) -> V {
            return k >= C ? Frag<T>::zero() : ldfrag<T>(oh + (size_t)m * lay.ldo + k);
        }, [&](int m, int col, float a) {
            const int n = n0 + m;
            if (col >= C) return;
            float x = 0.f;
            if (n < N) {
                const float r = f(rnd<T>(a + br[col]));
                x = fmaf(r, scr[col], shr[col]);
                if (!COND) x *= code_r[(size_t)n * C + col];
                if (l > 0) x += f(xc[(size_t)m * C + col]);
            }
            const T xt = rnd<T>(x);
            xc[(size_t)m * C + col] = xt;
            if (n < N && l + 1 < L) xh[(((size_t)l * N + n) * W + j) * C + col] = xt;
        });
        __syncthreads();
    }
    // head: 1x1 -> BN -> ReLU -> MC -> 1x1 (mcpixelcnn.py:85-88)
    const float* ph = P.p + g.p(L);
    const float *b0 = ph, *sc0 = ph + Hd, *sh0 = ph + 2 * Hd, *b4 = ph + 3 * Hd;
    const float* code0 = P.mc + (size_t)L * 3 * N * C;
    gemm<T>(M, r16(Hd), r32(C), wts + g.w0(), [&](int m, int k) -> V {
        return k >= C ? Frag<T>::zero() : ldfrag<T>(xc + (size_t)m * C + k);
    }, [&](int m, int col, float a) {
        if (col >= Hd) return;
        const int n = n0 + m;
        const float h = f(rnd<T>(a + b0[col]));
        zz[(size_t)m * lay.ldz + col] = rnd<T>(n < N ? fmaxf(fmaf(h, sc0[col], sh0[col]), 0.f) * (COND ? 1.f : code0[(size_t)n * Hd + col]) : 0.f);
    });
    __syncthreads();
    gemm<T>(M, r16(Kq), r32(Hd), wts + g.w4(), [&](int m, int k) -> V {
        return k >= Hd ? Frag<T>::zero() : ldfrag<T>(zz + (size_t)m * lay.ldz + k);
    }, [&](int m, int col, float a) {
        if (col >= Kq) return;
        const float v = f(rnd<T>(a + b4[col]));
        lg[m * Kq + col] = v;
        const int n = n0 + m;
        if (P.logits && n < N) P.logits[(((size_t)n * H + i) * W + j) * Kq + col] = v;
    });
    __syncthreads();
    // softmax in fp32 and the draw: one wave per sample, lane l owns the contiguous logits [l * per, (l + 1) * per)
    const int lane = tid & 63, wave = tid >> 6, per = (Kq + 63) / 64, k0 = lane * per, k1 = min(k0 + per, Kq);
    for (int m = wave; m < 16; m += PX_WAVES) {
        const int n = n0 + m;
        if (n >= N) break;
        const float* x = lg + m * Kq;
        float mx = -INFINITY; int am = Kq;
        for (int k = k0; k < k1; ++k) if (x[k] > mx) { mx = x[k]; am = k; }
        for (int o = 32; o > 0; o >>= 1) {            // max, first index among equals
            const float om = __shfl_xor(mx, o); const int oa = __shfl_xor(am, o);
            if (om > mx || (om == mx && oa < am)) { mx = om; am = oa; }
        }
        int pick = am;
        if (!P.greedy) {
            // inverse CDF in index order: the smallest k with sum_{m <= k} e_m > u * sum_m e_m, e_m = exp(x_m - max)
            float loc = 0.f; int last = -1;
            for (int k = k0; k < k1; ++k) { const float e = expf(x[k] - mx); loc += e; if (e > 0.f) last = k; }
            float inc = loc;
            for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(inc, o); if (lane >= o) inc += t; }
            const float tot = __shfl(inc, 63);
            const float target = P.uniform[(size_t)(i * W + j) * N + n] * tot;
            int hit = Kq;
            if (inc > target) {
                float run = inc - loc;
                hit = last >= 0 ? last : Kq;
                for (int k = k0; k < k1; ++k) { run += expf(x[k] - mx); if (run > target) { hit = k; break; } }
            }
            for (int o = 32; o > 0; o >>= 1) hit = min(hit, __shfl_xor(hit, o));
            int lastall = last;
            for (int o = 32; o > 0; o >>= 1) lastall = max(lastall, __shfl_xor(lastall, o));
            pick = hit < Kq ? hit : lastall;          // u * S rounded up to S: the last code with mass
        }
        if (lane == 0) P.codes[((size_t)n * H + i) * W + j] = pick < Kq ? pick : Kq - 1;
    }
}

int px_check(const mcgen_px_sample_t* p, int dtype) {
    MCGEN_CHECK(p && p->codes && p->emb && p->w && p->p && p->mc && p->ov && p->v2h && p->xh, "px_sample: null pointer");
    MCGEN_CHECK(p->N > 0 && p->H > 0 && p->W > 0 && p->L >= 1 && p->C > 0 && p->C % 8 == 0 && p->Hd > 0 && p->Hd % 8 == 0 &&
                p->Kq > 0, "px_sample: bad shape N %d H %d W %d C %d L %d Hd %d Kq %d", p->N, p->H, p->W, p->C, p->L, p->Hd, p->Kq);
    MCGEN_CHECK(dtype == 0 || dtype == 1, "px_sample: unknown dtype %d", dtype);
    return 0;
}
}  // namespace

extern "C" int64_t mcgen_px_sample_weight_elems(int C, int L, int Hd, int Kq) {
    const Geo g{C, L, Hd, Kq};
    return (int64_t)(g.w4() + (size_t)r16(Kq) * r32(Hd));
}

namespace {
template <bool COND>
int launch_row(const mcgen_px_sample_t* p, int i, int dtype, void* stream, const char* what) {
    if (int rc = px_check(p, dtype)) return rc;
    MCGEN_CHECK(i >= 0 && i < p->H, "%s: row %d outside [0, %d)", what, i, p->H);
    const RowLds lay(p->W, p->C, dtype ? 2 : 4);
    MCGEN_CHECK(lay.bytes <= (size_t)PX_LDS_MAX, "%s: %zu bytes of LDS for W %d C %d", what, lay.bytes, p->W, p->C);
    const void* k = dtype ? reinterpret_cast<const void*>(px_row_kernel<bf16_t, COND>) : reinterpret_cast<const void*>(px_row_kernel<float, COND>);
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lay.bytes);
    MCGEN_CHECK(e == hipSuccess, "%s: LDS attribute: %s", what, hipGetErrorString(e));
    const dim3 grid((p->N + lay.SR - 1) / lay.SR);
    if (dtype) hipLaunchKernelGGL((px_row_kernel<bf16_t, COND>), grid, dim3(PX_THREADS), lay.bytes, STREAM(stream), *p, i);
    else hipLaunchKernelGGL((px_row_kernel<float, COND>), grid, dim3(PX_THREADS), lay.bytes, STREAM(stream), *p, i);
    MCGEN_LAUNCH_CHECK(what); return 0;
}

template <bool COND>
int launch_col(const mcgen_px_sample_t* p, int i, int j, int dtype, void* stream, const char* what) {
    if (int rc = px_check(p, dtype)) return rc;
    MCGEN_CHECK(i >= 0 && i < p->H && j >= 0 && j < p->W && p->uniform, "%s: bad position (%d, %d) or no uniforms", what, i, j);
    const ColLds lay(p->C, p->Hd, p->Kq, dtype ? 2 : 4);
    MCGEN_CHECK(lay.bytes <= (size_t)PX_LDS_MAX, "%s: %zu bytes of LDS for C %d Hd %d Kq %d", what, lay.bytes, p->C, p->Hd, p->Kq);
    const void* k = dtype ? reinterpret_cast<const void*>(px_col_kernel<bf16_t, COND>) : reinterpret_cast<const void*>(px_col_kernel<float, COND>);
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lay.bytes);
    MCGEN_CHECK(e == hipSuccess, "%s: LDS attribute: %s", what, hipGetErrorString(e));
    const dim3 grid((p->N + 15) / 16);
    if (dtype) hipLaunchKernelGGL((px_col_kernel<bf16_t, COND>), grid, dim3(PX_THREADS), lay.bytes, STREAM(stream), *p, i, j);
    else hipLaunchKernelGGL((px_col_kernel<float, COND>), grid, dim3(PX_THREADS), lay.bytes, STREAM(stream), *p, i, j);
    MCGEN_LAUNCH_CHECK(what); return 0;
}
}  // namespace

extern "C" int mcgen_px_sample_row(const mcgen_px_sample_t* p, int i, int dtype, void* stream) {
    return launch_row<false>(p, i, dtype, stream, "px_sample_row");
}

extern "C" int mcgen_px_sample_col(const mcgen_px_sample_t* p, int i, int j, int dtype, void* stream) {
    return launch_col<false>(p, i, j, dtype, stream, "px_sample_col");
}

extern "C" int mcgen_cpx_sample_row(const mcgen_px_sample_t* p, int i, int dtype, void* stream) {
    return launch_row<true>(p, i, dtype, stream, "cpx_sample_row");
}

extern "C" int mcgen_cpx_sample_col(const mcgen_px_sample_t* p, int i, int j, int dtype, void* stream) {
    return launch_col<true>(p, i, j, dtype, stream, "cpx_sample_col");
}
