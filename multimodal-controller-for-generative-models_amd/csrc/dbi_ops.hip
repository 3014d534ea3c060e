// Davies-Bouldin index of labelled rows (gfx950): scikit-learn's davies_bouldin_score (the reference's metrics.py:164-166) on
// tensors that stay in HBM.  Rows x [N][D] fp32 are grouped by cluster through `order` (row ids sorted by cluster, stable)
// and `offset` ([K + 1] segment bounds into `order`).  Inputs are read as fp32, every sum is carried in fp64, and every
// reduction has a fixed order with no atomics, so a repeated call returns the same bits.
//   dbi_centroid_kernel   cent[k][d]  = mean of the cluster's rows                   (lanes take adjacent columns)
//   dbi_row_dist_kernel   dist[r]     = || x[order[r]] - cent[cluster of r] ||       (one workgroup per row)
//   dbi_spread_kernel     s[k]        = mean of dist over the cluster's segment
//   dbi_pair_kernel       16 x 16 tile of centroid pairs: M_kl = || c_k - c_l ||, ratio (s_k + s_l) / M_kl (M = 0 -> +inf),
//                         the tile's row maxima of ratio and of M
//   dbi_final_kernel      score = mean_k max_l ratio, max_k s_k, max_kl M_kl
// Entry points documented in include/mcgen_hip.h.
#include "mcgen_common.h"

namespace {
#define STREAM(s) reinterpret_cast<hipStream_t>(s)
constexpr int kCols = 64;        // columns per workgroup of the centroid kernel (one wave wide: coalesced 256-byte rows)
constexpr int kSlices = 4;       // row slices per workgroup of the centroid kernel
constexpr int kTile = 16;        // centroid pairs per side of a pair tile
constexpr int kChunk = 64;       // columns of both tile sides staged in LDS at a time
constexpr int kPitch = kChunk + 1;   // odd fp64 pitch: the 16 rows a wave reads at one column fall into distinct banks

// sum of the 256 per-thread values in a fixed tree order; every thread gets the result
__device__ __forceinline__ double block_sum_256(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double block_max_256(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = fmax(red[t], red[t + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// grid (ceil(D / 64), K), 256 threads = 64 columns x 4 row slices: slice j sums the segment's rows j, j + 4, ... in ascending
// order, the four slice sums are then added in slice order
__global__ __launch_bounds__(256) void dbi_centroid_kernel(const float* __restrict__ x, const int64_t* __restrict__ order,
                                                           const int64_t* __restrict__ offset, double* __restrict__ cent, int D) {
    __shared__ double part[kSlices][kCols];
    const int k = blockIdx.y, col = threadIdx.x % kCols, slice = threadIdx.x / kCols;
    const int d = blockIdx.x * kCols + col;
    const int64_t r0 = offset[k], r1 = offset[k + 1];
    double acc = 0.0;
    if (d < D)
        for (int64_t r = r0 + slice; r < r1; r += kSlices) acc += (double)x[(size_t)order[r] * D + d];
    part[slice][col] = acc;
    __syncthreads();
    if (slice == 0 && d < D) {
        double sum = part[0][col];
        for (int j = 1; j < kSlices; ++j) sum += part[j][col];
        cent[(size_t)k * D + d] = sum / (double)(r1 - r0);
    }
}

// grid N, 256 threads: sorted position r, its row order[r] and its cluster cluster[order[r]]
__global__ __launch_bounds__(256) void dbi_row_dist_kernel(const float* __restrict__ x, const int64_t* __restrict__ order,
                                                           const int64_t* __restrict__ cluster, const double* __restrict__ cent,
                                                           double* __restrict__ dist, int D) {
    __shared__ double red[256];
    const size_t row = (size_t)order[blockIdx.x];
    const float* xr = x + row * D;
    const double* c = cent + (size_t)cluster[row] * D;
    double acc = 0.0;
    for (int d = threadIdx.x; d < D; d += 256) {
        const double v = (double)xr[d] - c[d];
        acc += v * v;
    }
    const double sum = block_sum_256(acc, red);
    if (threadIdx.x == 0) dist[blockIdx.x] = sqrt(sum);
}

// grid K, 256 threads: the mean of dist over the cluster's segment
__global__ __launch_bounds__(256) void dbi_spread_kernel(const double* __restrict__ dist, const int64_t* __restrict__ offset,
                                                         double* __restrict__ spread) {
    __shared__ double red[256];
    const int64_t r0 = offset[blockIdx.x], r1 = offset[blockIdx.x + 1];
    double acc = 0.0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) acc += dist[r];
    const double sum = block_sum_256(acc, red);
    if (threadIdx.x == 0) spread[blockIdx.x] = sum / (double)(r1 - r0);
}

// grid (T, T) with T = ceil(K / 16), 256 threads: thread (i, j) owns the pair (k0 + i, l0 + j).  Rows past K are staged as
// zeros and never written.  tile_ratio / tile_m [K][T]: the maxima over the tile's columns, taken in ascending l.
__global__ __launch_bounds__(256) void dbi_pair_kernel(const double* __restrict__ cent, const double* __restrict__ spread,
                                                       double* __restrict__ tile_ratio, double* __restrict__ tile_m, int K, int D,
                                                       int T) {
    __shared__ double a[kTile][kPitch], b[kTile][kPitch];
    __shared__ double ratio[kTile][kTile + 1], dist[kTile][kTile + 1];
    const int k0 = blockIdx.y * kTile, l0 = blockIdx.x * kTile;
    const int i = threadIdx.x / kTile, j = threadIdx.x % kTile;
    double acc = 0.0;
    for (int d0 = 0; d0 < D; d0 += kChunk) {
        // stage: 16 rows x 64 columns per side, lanes along the columns
        for (int e = threadIdx.x; e < kTile * kChunk; e += 256) {
            const int row = e / kChunk, col = e % kChunk, d = d0 + col;
            const bool in = d < D;
            a[row][col] = (in && k0 + row < K) ? cent[(size_t)(k0 + row) * D + d] : 0.0;
            b[row][col] = (in && l0 + row < K) ? cent[(size_t)(l0 + row) * D + d] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int col = 0; col < kChunk; ++col) {
            const double v = a[i][col] - b[j][col];
            acc += v * v;
        }
        __syncthreads();
    }
    const int k = k0 + i, l = l0 + j;
    const bool live = k < K && l < K;
    const double m = sqrt(acc);
    dist[i][j] = live ? m : 0.0;
    ratio[i][j] = (live && m != 0.0) ? (spread[k] + spread[l]) / m : 0.0;      // M = 0 counts as +inf: the ratio is 0
    __syncthreads();
    if (threadIdx.x < kTile && k0 + (int)threadIdx.x < K) {
        const int row = threadIdx.x;
        double rmax = ratio[row][0], mmax = dist[row][0];
        for (int c = 1; c < kTile; ++c) { rmax = fmax(rmax, ratio[row][c]); mmax = fmax(mmax, dist[row][c]); }
        tile_ratio[(size_t)(k0 + row) * T + blockIdx.x] = rmax;
        tile_m[(size_t)(k0 + row) * T + blockIdx.x] = mmax;
    }
}

// one workgroup: out[0] = mean_k max_tiles ratio, out[1] = max_k spread, out[2] = max over all pairs of M
__global__ __launch_bounds__(256) void dbi_final_kernel(const double* __restrict__ tile_ratio, const double* __restrict__ tile_m,
                                                        const double* __restrict__ spread, double* __restrict__ out, int K, int T) {
    __shared__ double red[256];
    double sum = 0.0, smax = 0.0, mmax = 0.0;
    for (int k = threadIdx.x; k < K; k += 256) {
        double rmax = tile_ratio[(size_t)k * T];
        for (int t = 0; t < T; ++t) {
            rmax = fmax(rmax, tile_ratio[(size_t)k * T + t]);
            mmax = fmax(mmax, tile_m[(size_t)k * T + t]);
        }
        sum += rmax;
        smax = fmax(smax, spread[k]);
    }
    const double total = block_sum_256(sum, red);
    const double s_all = block_max_256(smax, red);
    const double m_all = block_max_256(mmax, red);
    if (threadIdx.x == 0) { out[0] = total / (double)K; out[1] = s_all; out[2] = m_all; }
}
}  // namespace

extern "C" int mcgen_dbi_centroids(const float* x, const int64_t* order, const int64_t* offset, double* cent, int64_t N, int D,
                                   int K, void* stream) {
    MCGEN_CHECK(x && order && offset && cent && N > 0 && D > 0 && K > 0 && K <= 65535 && K <= N, "dbi_centroids: bad arguments");
    hipLaunchKernelGGL(dbi_centroid_kernel, dim3((D + kCols - 1) / kCols, K), dim3(256), 0, STREAM(stream), x, order, offset, cent, D);
    MCGEN_LAUNCH_CHECK("dbi_centroids"); return 0;
}

extern "C" int mcgen_dbi_spread(const float* x, const int64_t* order, const int64_t* cluster, const int64_t* offset,
                                const double* cent, double* dist, double* spread, int64_t N, int D, int K, void* stream) {
    MCGEN_CHECK(x && order && cluster && offset && cent && dist && spread && N > 0 && N < (1ll << 31) && D > 0 && K > 0 && K <= N,
                "dbi_spread: bad arguments");
    hipLaunchKernelGGL(dbi_row_dist_kernel, dim3((unsigned)N), dim3(256), 0, STREAM(stream), x, order, cluster, cent, dist, D);
    MCGEN_LAUNCH_CHECK("dbi_row_dist");
    hipLaunchKernelGGL(dbi_spread_kernel, dim3(K), dim3(256), 0, STREAM(stream), dist, offset, spread);
    MCGEN_LAUNCH_CHECK("dbi_spread"); return 0;
}

extern "C" int mcgen_dbi_tiles(int K) { return K > 0 ? (K + kTile - 1) / kTile : 0; }

extern "C" int mcgen_dbi_score(const double* cent, const double* spread, double* tile_ratio, double* tile_m, double* out, int D,
                               int K, void* stream) {
    MCGEN_CHECK(cent && spread && tile_ratio && tile_m && out && D > 0 && K > 0 && K <= 65535 * kTile, "dbi_score: bad arguments");
    const int T = mcgen_dbi_tiles(K);
    hipLaunchKernelGGL(dbi_pair_kernel, dim3(T, T), dim3(256), 0, STREAM(stream), cent, spread, tile_ratio, tile_m, K, D, T);
    MCGEN_LAUNCH_CHECK("dbi_pair");
    hipLaunchKernelGGL(dbi_final_kernel, dim3(1), dim3(256), 0, STREAM(stream), tile_ratio, tile_m, spread, out, K, T);
    MCGEN_LAUNCH_CHECK("dbi_final"); return 0;
}
