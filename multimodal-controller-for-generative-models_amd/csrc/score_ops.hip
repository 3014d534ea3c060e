// Streaming accumulators behind Inception Score and FID (gfx950): what metrics.inception_score / metrics.fid get from one
// concatenated float64 matrix each, as sums a batch adds to --
//   psum[c] += sum_rows softmax(logits)[row, c],   plogp[0] += sum_rows sum_c p log p          (mcgen_score_probs)
//   fsum[j] += sum_rows x[row, j],                 gram[i, j] += sum_rows x[row, i] x[row, j]  (mcgen_score_moments)
// Inputs are read as fp32 and widened; every sum, exp and log is fp64.  No atomics, and every reduction has an order fixed by
// the shapes alone, so a repeated call returns the same bits:
//   score_probs_kernel        a wave owns a contiguous ascending slice of rows and takes them one at a time, lanes along the
//                             classes: row maximum and exp sum by a butterfly over the 64 lanes, then p = exp(x - max) / Z is
//                             added to the slice's own column partials in `work` (a lane owns its columns: plain read-add-write,
//                             the first row writes), p (x - max - log Z) to the lane's entropy sum
//   score_probs_final_kernel  thread c adds column c of the slices in ascending slice order, then psum[c] += / plogp[0] +=
//   score_gram_kernel         one workgroup per 64 x 64 tile of the upper triangle, a wave per 16 x 32 part = two
//                             v_mfma_f64_16x16x4_f64 accumulators; it walks all n rows ascending, four rows per MFMA step, the
//                             operands straight from global memory (rows beyond n and columns beyond D enter as zeros), so
//                             nothing is reduced between workgroups.  A tile is added at (i, j) and, transposed, at (j, i);
//                             a diagonal tile keeps its elements with i <= j and mirrors those, so gram stays bitwise symmetric
//   score_colsum_kernel       thread per column, a contiguous slab of rows ascending -> the slab's partial in `work`
//   score_colsum_final_kernel thread j adds column j of the slabs in ascending order, then fsum[j] +=
// Entry points documented in include/mcgen_hip.h.
#include "mcgen_common.h"

namespace {
#define STREAM(s) reinterpret_cast<hipStream_t>(s)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlices = 256;                   // most row slices of score_probs (one wave each)
constexpr int kSliceRows = 4;                  // rows a slice has before the number of slices stops growing
constexpr int kSlabs = 128;                    // most row slabs of the column sums
constexpr int kSlabRows = 32;
constexpr int kTile = 64;                      // gram tile per workgroup
constexpr int kGramThreads = 512;              // eight waves, a 16 x 32 part of the tile each

typedef double f64x4 __attribute__((ext_vector_type(4)));

// rows per part and number of parts (none empty): `most` parts at the most, `least` rows each at the least
static void split_rows(int64_t n, int most, int least, int64_t& rows, int& parts) {
    rows = (n + most - 1) / most;
    if (rows < least) rows = least;
    parts = (int)((n + rows - 1) / rows);
}

// ---- class probabilities ---------------------------------------------------------------------------------------------------
// grid ceil(S / 4) x 256: wave s < S owns rows s * R .. min(n, (s + 1) * R) - 1 and work[s][0 .. C] (C column sums, then its
// sum of p log p).  A NaN in a row makes Z, hence every p of the row, NaN; p == 0 contributes 0.
__global__ __launch_bounds__(kThreads) void score_probs_kernel(const float* __restrict__ logits, int64_t n, int C, int64_t R, int S,
                                                               double* __restrict__ work) {
    const int lane = threadIdx.x & 63, s = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (s >= S) return;
    double* __restrict__ part = work + (int64_t)s * (C + 1);
    const int64_t first = (int64_t)s * R, last = first + R < n ? first + R : n;
    double ent = 0.0;
    for (int64_t r = first; r < last; ++r) {
        const float* __restrict__ x = logits + r * C;
        float m = -__builtin_inff();
        for (int c = lane; c < C; c += 64) m = fmaxf(m, x[c]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        const double md = (double)m;
        double z = 0.0;
        for (int c = lane; c < C; c += 64) z += exp((double)x[c] - md);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off);          // a + b on both sides: every lane holds the same bits
        const double lz = log(z);
        for (int c = lane; c < C; c += 64) {
            const double d = (double)x[c] - md;
            const double p = exp(d) / z;
            ent += p == 0.0 ? 0.0 : p * (d - lz);                                // log p = x - max - log Z;  0 log 0 = 0
            part[c] = r == first ? p : part[c] + p;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ent += __shfl_down(ent, off);
    if (lane == 0) part[C] = ent;
}

__global__ __launch_bounds__(kThreads) void score_probs_final_kernel(const double* __restrict__ work, int S, int C,
                                                                     double* __restrict__ psum, double* __restrict__ plogp) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j > C) return;
    double sum = work[j];
    for (int s = 1; s < S; ++s) sum += work[(int64_t)s * (C + 1) + j];
    if (j < C) psum[j] += sum; else plogp[0] += sum;
}

// ---- feature moments -------------------------------------------------------------------------------------------------------
// grid (ceil(D / 256), S) x 256: thread = column j, block row s = rows s * R .. ; work[s][j] = the slab's column sum
__global__ __launch_bounds__(kThreads) void score_colsum_kernel(const float* __restrict__ x, int64_t n, int D, int64_t R,
                                                                double* __restrict__ work) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= D) return;
    const int64_t first = (int64_t)blockIdx.y * R, last = first + R < n ? first + R : n;
    double sum = 0.0;
#pragma unroll 4
    for (int64_t r = first; r < last; ++r) sum += (double)x[r * D + j];
    work[(int64_t)blockIdx.y * D + j] = sum;
}

__global__ __launch_bounds__(kThreads) void score_colsum_final_kernel(const double* __restrict__ work, int S, int D,
                                                                      double* __restrict__ fsum) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= D) return;
    double sum = work[j];
    for (int s = 1; s < S; ++s) sum += work[(int64_t)s * D + j];
    fsum[j] += sum;
}

// grid (T, T) x 512, T = ceil(D / 64); block (x = tj, y = ti) with ti <= tj works, the others leave.  Wave w of the eight owns
// rows 16 (w >> 1) .. + 15 and columns 32 (w & 1) .. + 31 of the tile: two accumulators side by side.  v_mfma_f64_16x16x4_f64:
// lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] (one fp64 each) and holds D[i = (l >> 4) + 4 reg]
// [j = l & 15], reg = 0 .. 3.  Here A[i][k] = x[r0 + k][i0 + i] and B[k][j] = x[r0 + k][j0 + j]: both operands are the lane's
// row r0 + (l >> 4) at a column of the i side and of the j side.  Sixteen rows (four MFMA steps) are in flight while the
// previous sixteen are multiplied: two register buffers, filled and used in turn.
struct GramRows { float a[4], b[4][2]; };

__device__ __forceinline__ void gram_load(GramRows& f, const float* pa, const float* pb0, const float* pb1, int64_t row, int D) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t at = (row + 4 * k) * D;
        f.a[k] = pa[at];  f.b[k][0] = pb0[at];  f.b[k][1] = pb1[at];
    }
}

__device__ __forceinline__ void gram_mfma(const GramRows& f, bool ma, bool mb0, bool mb1, f64x4 (&acc)[2]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double a = ma ? (double)f.a[k] : 0.0;
        const double b0 = mb0 ? (double)f.b[k][0] : 0.0, b1 = mb1 ? (double)f.b[k][1] : 0.0;
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[1], 0, 0, 0);
    }
}

__global__ __launch_bounds__(kGramThreads) void score_gram_kernel(const float* __restrict__ x, int64_t n, int D, double* __restrict__ gram) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const bool diag = ti == tj;
    if (diag && wi * 16 >= (wj + 1) * 32) return;                     // wholly below the diagonal: mirrored from above it
    const int i0 = ti * kTile + wi * 16, j0 = tj * kTile + wj * 32;
    const int lc = lane & 15, lk = lane >> 4;
    // a column beyond D reads column 0 instead and enters as zero
    const int ca = i0 + lc, cb[2] = {j0 + lc, j0 + 16 + lc};
    const bool ma = ca < D, mb[2] = {cb[0] < D, cb[1] < D};
    const float* pa = x + (ma ? ca : 0);
    const float* pb[2] = {x + (mb[0] ? cb[0] : 0), x + (mb[1] ? cb[1] : 0)};
    f64x4 acc[2] = {f64x4{0.0, 0.0, 0.0, 0.0}, f64x4{0.0, 0.0, 0.0, 0.0}};
    const int64_t blocks = n & ~(int64_t)31;                          // rows in whole blocks of thirty-two: two buffers of sixteen
    GramRows even, odd;
    if (blocks > 0) gram_load(even, pa, pb[0], pb[1], lk, D);
    for (int64_t r0 = 0; r0 < blocks; r0 += 32) {
        gram_load(odd, pa, pb[0], pb[1], r0 + 16 + lk, D);
        gram_mfma(even, ma, mb[0], mb[1], acc);
        gram_load(even, pa, pb[0], pb[1], (r0 + 32 < blocks ? r0 + 32 : r0) + lk, D);      // (after the last block: loaded, not used)
        gram_mfma(odd, ma, mb[0], mb[1], acc);
    }
    for (int64_t r0 = blocks; r0 < n; r0 += 4) {                      // the last steps: a row beyond n reads row 0 and enters as zero
        const bool in = r0 + lk < n;
        const int64_t at = in ? (r0 + lk) * D : 0;
        const double a = in && ma ? (double)pa[at] : 0.0;
        const double b0 = in && mb[0] ? (double)pb[0][at] : 0.0, b1 = in && mb[1] ? (double)pb[1][at] : 0.0;
        acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[1], 0, 0, 0);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int i = i0 + lk + 4 * reg, j = j0 + b * 16 + lc;
            if (i >= D || j >= D || (diag && i > j)) continue;
            const double v = acc[b][reg];
            gram[(int64_t)i * D + j] += v;
            if (i != j) gram[(int64_t)j * D + i] += v;
        }
}
}  // namespace

extern "C" int64_t mcgen_score_probs_work(int64_t n, int C) {
    if (n < 1 || C < 2 || C > 65535) return 0;
    int64_t rows; int parts;
    split_rows(n, kSlices, kSliceRows, rows, parts);
    return (int64_t)parts * (C + 1);
}

extern "C" int mcgen_score_probs(const float* logits, int64_t n, int C, double* work, double* psum, double* plogp, void* stream) {
    MCGEN_CHECK(logits && work && psum && plogp && n >= 1, "score_probs: bad arguments");
    MCGEN_CHECK(C >= 2 && C <= 65535, "score_probs: %d classes outside [2, 65535]", C);
    int64_t R; int S;
    split_rows(n, kSlices, kSliceRows, R, S);
    hipLaunchKernelGGL(score_probs_kernel, dim3((S + kWaves - 1) / kWaves), dim3(kThreads), 0, STREAM(stream), logits, n, C, R, S, work);
    MCGEN_LAUNCH_CHECK("score_probs");
    hipLaunchKernelGGL(score_probs_final_kernel, dim3(C / kThreads + 1), dim3(kThreads), 0, STREAM(stream), work, S, C, psum, plogp);
    MCGEN_LAUNCH_CHECK("score_probs_final"); return 0;
}

extern "C" int64_t mcgen_score_moments_work(int64_t n, int D) {
    if (n < 1 || D < 1 || D > 65535) return 0;
    int64_t rows; int parts;
    split_rows(n, kSlabs, kSlabRows, rows, parts);
    return (int64_t)parts * D;
}

extern "C" int mcgen_score_moments(const float* feat, int64_t n, int D, double* work, double* fsum, double* gram, void* stream) {
    MCGEN_CHECK(feat && work && fsum && gram && n >= 1, "score_moments: bad arguments");
    MCGEN_CHECK(D >= 1 && D <= 65535, "score_moments: %d columns outside [1, 65535]", D);
    int64_t R; int S;
    split_rows(n, kSlabs, kSlabRows, R, S);
    const int cols = (D + kThreads - 1) / kThreads, T = (D + kTile - 1) / kTile;
    hipLaunchKernelGGL(score_colsum_kernel, dim3(cols, S), dim3(kThreads), 0, STREAM(stream), feat, n, D, R, work);
    MCGEN_LAUNCH_CHECK("score_colsum");
    hipLaunchKernelGGL(score_colsum_final_kernel, dim3(cols), dim3(kThreads), 0, STREAM(stream), work, S, D, fsum);
    MCGEN_LAUNCH_CHECK("score_colsum_final");
    hipLaunchKernelGGL(score_gram_kernel, dim3(T, T), dim3(kGramThreads), 0, STREAM(stream), feat, n, D, gram);
    MCGEN_LAUNCH_CHECK("score_gram"); return 0;
}
