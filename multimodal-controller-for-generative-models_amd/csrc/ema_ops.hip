// libmcgen_hip.so -- the averaged generator (trainer.FusedEMA): an exponential moving average over a flat fp32 range and
// an in-place exchange of two ranges, one launch each.
//
// Both kernels are HBM/L2 streams in the style of optim_ops.hip: every lane moves 16 bytes per access (f32x4), a trip of
// the main loop issues the loads of two vectors of both ranges before it computes, the grid is capped and strides.  No LDS.
// The ranges are sub-ranges of flat buffers and may start at any element: when both bases sit at the SAME offset inside
// their 16-byte lines, `head` (0..3) scalar elements bring them to a line start, the f32x4 loops cover the next 4 * nv
// elements and a scalar loop the rest; when the offsets differ there is no vector part (nv = 0) and the scalar loop covers
// all n elements.
//
// The step count of mcgen_ema_update is read from device memory when the kernel runs (a captured launch stays valid
// across iterations) and advanced by the launch that passes advance = 1: its blocks end on the {counter, ticket} pair of
// mcgen_adam, the last one to finish increments the counter -- every block of the launch has read it by then.  A launch
// with advance = 0 touches no atomic at all.
#include "mcgen_common.h"

namespace {

constexpr int EMA_BLOCK = 256;
// A launch that ends on the step ticket keeps optim_ops.hip's cap of one block per CU (the tickets serialize on one
// address); a launch without it takes the usual cap of a memory-bound stream, 8 blocks per CU.
constexpr int EMA_GRID_TICKET = 256;
constexpr int EMA_GRID_STREAM = 2048;
#define STREAM(s) reinterpret_cast<hipStream_t>(s)

struct EmaOp {
    float d, omd;          // decay, 1 - decay (fp32)
    bool copy;             // still inside the warm-up: the average follows the parameters bit for bit
    __device__ __forceinline__ void operator()(float& e, float& p) const { e = copy ? p : fmaf(d, e, omd * p); }
    static constexpr bool WRITES_B = false;
};
struct SwapOp {
    __device__ __forceinline__ void operator()(float& a, float& b) const { const float t = a; a = b; b = t; }
    static constexpr bool WRITES_B = true;
};

// a[k], b[k] <- op(a[k], b[k]) for k in [0, n): elements [0, head) and [head + 4 nv, n) one by one, the rest as f32x4
template <typename Op>
__device__ __forceinline__ void pair_stream(const Op& op, float* __restrict__ a, float* __restrict__ b, size_t n, size_t head, size_t nv) {
    f32x4* a4 = reinterpret_cast<f32x4*>(a + head);
    f32x4* b4 = reinterpret_cast<f32x4*>(b + head);
    const size_t st = (size_t)gridDim.x * blockDim.x;
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    size_t i = gid;
    for (; i + st < nv; i += 2 * st) {
        f32x4 av[2], bv[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) { av[e] = a4[i + e * st]; bv[e] = b4[i + e * st]; }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
#pragma unroll
            for (int c = 0; c < 4; ++c) { float x = av[e][c], y = bv[e][c]; op(x, y); av[e][c] = x; bv[e][c] = y; }
            a4[i + e * st] = av[e];
            if (Op::WRITES_B) b4[i + e * st] = bv[e];
        }
    }
    for (; i < nv; i += st) {
        f32x4 av = a4[i], bv = b4[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) { float x = av[c], y = bv[c]; op(x, y); av[c] = x; bv[c] = y; }
        a4[i] = av;
        if (Op::WRITES_B) b4[i] = bv;
    }
    // the scalar elements: `head` in front of the vectors and n - head - 4 nv behind them
    const size_t ns = n - 4 * nv;
    for (size_t k = gid; k < ns; k += st) {
        const size_t j = k < head ? k : k + 4 * nv;
        float x = a[j], y = b[j];
        op(x, y);
        a[j] = x;
        if (Op::WRITES_B) b[j] = y;
    }
}

__global__ __launch_bounds__(EMA_BLOCK) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, size_t n, size_t head,
                                                               size_t nv, float d, int64_t start, int64_t* step, int advance) {
    const int64_t t = step[0];           // updates done so far, read at execution time
    pair_stream(EmaOp{d, 1.0f - d, t < start}, ema, const_cast<float*>(p), n, head, nv);
    if (advance) {                       // (uniform over the launch)
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned* ticket = reinterpret_cast<unsigned*>(step + 1);
            const unsigned prev = atomicAdd(ticket, 1u);
            if (prev == gridDim.x - 1) { *ticket = 0u; step[0] = t + 1; }
        }
    }
}

__global__ __launch_bounds__(EMA_BLOCK) void swap_kernel(float* __restrict__ a, float* __restrict__ b, size_t n, size_t head, size_t nv) {
    pair_stream(SwapOp{}, a, b, n, head, nv);
}

// (head, nv) of a pair of ranges: see the top of the file
inline void pair_split(const void* a, const void* b, int64_t n, size_t* head, size_t* nv) {
    const uintptr_t oa = reinterpret_cast<uintptr_t>(a) & 15, ob = reinterpret_cast<uintptr_t>(b) & 15;
    *head = 0; *nv = 0;
    if (oa != ob) return;
    size_t h = ((16 - oa) & 15) / 4;
    if (h > (size_t)n) h = (size_t)n;
    *head = h;
    *nv = ((size_t)n - h) / 4;
}
inline int pair_grid(size_t n, size_t nv, int cap) {
    const size_t work = nv ? nv : n;                       // (at most 6 scalar elements go with nv vectors)
    size_t b = (work + EMA_BLOCK - 1) / EMA_BLOCK;
    if (b < 1) b = 1;
    if (b > (size_t)cap) b = cap;
    return (int)b;
}
inline bool aligned4(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 3) == 0; }

}  // namespace

extern "C" int mcgen_ema_update(float* ema, const float* p, int64_t n, float decay, int64_t start, int64_t* step, int advance,
                                void* stream) {
    MCGEN_CHECK(ema && p && step && n > 0, "ema_update: bad arguments (step: int64[2] = {counter, ticket = 0})");
    MCGEN_CHECK(aligned4(ema) && aligned4(p), "ema_update: the ranges must be 4-byte aligned");
    MCGEN_CHECK(decay >= 0.f && decay <= 1.f && start >= 0, "ema_update: decay in [0, 1] and start >= 0");
    MCGEN_CHECK(ema + n <= p || p + n <= ema, "ema_update: the ranges overlap");
    size_t head, nv;
    pair_split(ema, p, n, &head, &nv);
    const int grid = pair_grid((size_t)n, nv, advance ? EMA_GRID_TICKET : EMA_GRID_STREAM);
    hipLaunchKernelGGL(ema_update_kernel, dim3(grid), dim3(EMA_BLOCK), 0, STREAM(stream), ema, p, (size_t)n, head, nv, decay, start, step,
                       advance ? 1 : 0);
    MCGEN_LAUNCH_CHECK("ema_update"); return 0;
}

extern "C" int mcgen_swap_f32(float* a, float* b, int64_t n, void* stream) {
    MCGEN_CHECK(a && b && n > 0, "swap_f32: bad arguments");
    MCGEN_CHECK(aligned4(a) && aligned4(b), "swap_f32: the ranges must be 4-byte aligned");
    MCGEN_CHECK(a + n <= b || b + n <= a, "swap_f32: the ranges overlap");
    size_t head, nv;
    pair_split(a, b, n, &head, &nv);
    hipLaunchKernelGGL(swap_kernel, dim3(pair_grid((size_t)n, nv, EMA_GRID_STREAM)), dim3(EMA_BLOCK), 0, STREAM(stream), a, b, (size_t)n,
                       head, nv);
    MCGEN_LAUNCH_CHECK("swap_f32"); return 0;
}
