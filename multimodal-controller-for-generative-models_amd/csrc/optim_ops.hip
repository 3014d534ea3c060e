// libmcgen_hip.so -- the optimizers of cfg['optimizer_name'] besides Adam (train_gan.py:222-236, train_vae.py:151-165):
// SGD with momentum, RMSprop and Adamax over one flat fp32 buffer, torch.optim's single-tensor arithmetic, one launch
// per step.  mcgen_adam's contract (small_ops.hip): the learning rate is an immediate or one float in device memory
// read when the kernel runs; step = int64[2] {counter, ticket}, the counter advanced by the last block to finish.
//
// The kernels are HBM streams: every lane moves 16 bytes per access (f32x4) and a trip of the main loop issues the loads
// of two vectors of every stream before it computes; the grid is capped at OPT_GRID_CAP blocks and strides.  The vector
// loops cover the first 4 * nv elements (nv = n / 4 when every pointer is 16-byte aligned, else 0), a scalar loop the rest.
#include "mcgen_common.h"

namespace {

constexpr int OPT_BLOCK = 256;
// Blocks at most: one per CU.  Every block ends on the step ticket, an atomic on ONE address, and those serialize at about
// 11 ns each: at the CIFAR-10 generator's size a launch took 27 us (SGD) to 31 us (Adamax) with 2048 blocks and 8.5 to 19 us
// with 256, cache-resident or not.  Above 4 * 256 * 256 elements the two-vector loop runs.
#ifndef MCGEN_OPT_GRID_CAP
#define MCGEN_OPT_GRID_CAP 256
#endif
constexpr int OPT_GRID_CAP = MCGEN_OPT_GRID_CAP;
#define STREAM(s) reinterpret_cast<hipStream_t>(s)

// the step ticket and the integer power of mcgen_adam (small_ops.hip: adam_step_ticket, adam_powi), restated
__device__ __forceinline__ void optim_step_ticket(int64_t* step, unsigned total_blocks) {
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned* ticket = reinterpret_cast<unsigned*>(step + 1);
        const unsigned prev = atomicAdd(ticket, 1u);
        if (prev == total_blocks - 1) { *ticket = 0u; step[0] += 1; }
    }
}
__device__ __forceinline__ double optim_powi(double b, long t) {
    double r = 1.0;
    while (t > 0) { if (t & 1) r *= b; b *= b; t >>= 1; }
    return r;
}

// ---- the three updates, one element each: (p, g, s0, s1) -> (p, s0, s1) ----------------------------------------------
// torch.optim.SGD (no dampening, no Nesterov): buf = mu buf + g'; p -= lr buf.  From a zero buffer the first step gives
// buf = g', torch's first-step clone.  BUF = false (mu = 0): p -= lr g', no state.
template <bool BUF> struct SgdOp {
    static constexpr int NSTATE = BUF ? 1 : 0;
    float lr, mu, wd;
    __device__ __forceinline__ void operator()(float& p, float g, float& buf, float&) const {
        if (wd != 0.f) g = fmaf(wd, p, g);
        if (BUF) { buf = fmaf(mu, buf, g); g = buf; }
        p = fmaf(-lr, g, p);
    }
};
// torch.optim.RMSprop (not centered): sq = alpha sq + (1 - alpha) g'^2; avg = sqrt(sq) + eps;
// mu > 0: buf = mu buf + g' / avg, p -= lr buf;  mu = 0 (BUF = false): p -= lr g' / avg.
template <bool BUF> struct RmspropOp {
    static constexpr int NSTATE = BUF ? 2 : 1;
    float lr, alpha, eps, mu, wd;
    __device__ __forceinline__ void operator()(float& p, float g, float& sq, float& buf) const {
        if (wd != 0.f) g = fmaf(wd, p, g);
        sq = fmaf(alpha, sq, (1.f - alpha) * g * g);
        float q = g / (sqrtf(sq) + eps);
        if (BUF) { buf = fmaf(mu, buf, q); q = buf; }
        p = fmaf(-lr, q, p);
    }
};
// torch.optim.Adamax: m = b1 m + (1 - b1) g'; u = max(b2 u, |g'| + eps); p -= lr / (1 - b1^t) m / u  (clr = lr / bc1)
struct AdamaxOp {
    static constexpr int NSTATE = 2;
    float clr, b1, b2, eps, wd;
    __device__ __forceinline__ void operator()(float& p, float g, float& m, float& u) const {
        if (wd != 0.f) g = fmaf(wd, p, g);
        m = fmaf(b1, m, (1.f - b1) * g);
        u = fmaxf(b2 * u, fabsf(g) + eps);
        p = fmaf(-clr, m / u, p);
    }
};

template <typename Op>
__device__ __forceinline__ void optim_stream(const Op& op, float* __restrict__ p, const float* __restrict__ g,
                                             float* __restrict__ s0, float* __restrict__ s1, size_t n, size_t nv) {
    constexpr int NS = Op::NSTATE;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* a4 = reinterpret_cast<f32x4*>(s0);
    f32x4* b4 = reinterpret_cast<f32x4*>(s1);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const size_t st = (size_t)gridDim.x * blockDim.x;
    const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    size_t i = gid;
    // two vectors per trip, all loads of the trip first
    for (; i + st < nv; i += 2 * st) {
        f32x4 pv[2], gv[2], av[2], bv[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const size_t k = i + e * st;
            gv[e] = g4[k]; pv[e] = p4[k];
            av[e] = NS >= 1 ? a4[k] : zero;
            bv[e] = NS >= 2 ? b4[k] : zero;
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const size_t k = i + e * st;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float pc = pv[e][c], ac = av[e][c], bc = bv[e][c];
                op(pc, gv[e][c], ac, bc);
                pv[e][c] = pc; av[e][c] = ac; bv[e][c] = bc;
            }
            p4[k] = pv[e];
            if (NS >= 1) a4[k] = av[e];
            if (NS >= 2) b4[k] = bv[e];
        }
    }
    for (; i < nv; i += st) {
        f32x4 gv = g4[i], pv = p4[i];
        f32x4 av = NS >= 1 ? a4[i] : zero;
        f32x4 bv = NS >= 2 ? b4[i] : zero;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float pc = pv[c], ac = av[c], bc = bv[c];
            op(pc, gv[c], ac, bc);
            pv[c] = pc; av[c] = ac; bv[c] = bc;
        }
        p4[i] = pv;
        if (NS >= 1) a4[i] = av;
        if (NS >= 2) b4[i] = bv;
    }
    // the elements behind the last whole vector (all of them when a pointer is not 16-byte aligned)
    for (size_t k = 4 * nv + gid; k < n; k += st) {
        float pk = p[k], ak = NS >= 1 ? s0[k] : 0.f, bk = NS >= 2 ? s1[k] : 0.f;
        op(pk, g[k], ak, bk);
        p[k] = pk;
        if (NS >= 1) s0[k] = ak;
        if (NS >= 2) s1[k] = bk;
    }
}

template <bool BUF>
__global__ __launch_bounds__(OPT_BLOCK) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                        size_t n, size_t nv, float lr, const float* __restrict__ lr_dev,
                                                        float mu, float wd, int64_t* step) {
    if (lr_dev) lr = lr_dev[0];          // learning rate read at execution time: a captured launch follows a scheduler
    optim_stream(SgdOp<BUF>{lr, mu, wd}, p, g, buf, nullptr, n, nv);
    optim_step_ticket(step, gridDim.x);
}

template <bool BUF>
__global__ __launch_bounds__(OPT_BLOCK) void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq,
                                                            float* __restrict__ buf, size_t n, size_t nv, float lr,
                                                            const float* __restrict__ lr_dev, float alpha, float eps, float mu,
                                                            float wd, int64_t* step) {
    if (lr_dev) lr = lr_dev[0];
    optim_stream(RmspropOp<BUF>{lr, alpha, eps, mu, wd}, p, g, sq, buf, n, nv);
    optim_step_ticket(step, gridDim.x);
}

__global__ __launch_bounds__(OPT_BLOCK) void adamax_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ u, size_t n, size_t nv, float lr,
                                                           const float* __restrict__ lr_dev, float b1, float b2, float eps,
                                                           float wd, int64_t* step) {
    if (lr_dev) lr = lr_dev[0];
    const long t = (long)step[0] + 1;
    const float bc1 = (float)(1.0 - optim_powi((double)b1, t));
    optim_stream(AdamaxOp{lr / bc1, b1, b2, eps, wd}, p, g, m, u, n, nv);
    optim_step_ticket(step, gridDim.x);
}

inline bool aligned16(const void* a) { return a == nullptr || (reinterpret_cast<uintptr_t>(a) & 15) == 0; }
// vectors the f32x4 loops cover
inline size_t optim_vectors(int64_t n, const void* a, const void* b, const void* c, const void* d) {
    return aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d) ? (size_t)n / 4 : 0;
}
inline int optim_grid(size_t n, size_t nv) {
    const size_t work = nv ? nv : n;                       // (the scalar loop behind nv vectors has at most 3 elements)
    size_t b = (work + OPT_BLOCK - 1) / OPT_BLOCK;
    if (b < 1) b = 1;
    if (b > (size_t)OPT_GRID_CAP) b = OPT_GRID_CAP;
    return (int)b;
}

}  // namespace

extern "C" int mcgen_sgd(float* p, const float* g, float* buf, int64_t n, float lr, const float* lr_dev, float momentum,
                         float weight_decay, int64_t* step, void* stream) {
    MCGEN_CHECK(p && g && step && n > 0, "sgd: bad arguments (step: int64[2] = {counter, ticket = 0})");
    MCGEN_CHECK(momentum >= 0.f && (buf != nullptr) == (momentum != 0.f), "sgd: buf goes with momentum > 0 (NULL when momentum = 0)");
    const size_t nv = optim_vectors(n, p, g, buf, nullptr);
    const dim3 grid(optim_grid((size_t)n, nv)), block(OPT_BLOCK);
    if (buf) hipLaunchKernelGGL(sgd_kernel<true>, grid, block, 0, STREAM(stream), p, g, buf, (size_t)n, nv, lr, lr_dev, momentum, weight_decay, step);
    else hipLaunchKernelGGL(sgd_kernel<false>, grid, block, 0, STREAM(stream), p, g, buf, (size_t)n, nv, lr, lr_dev, momentum, weight_decay, step);
    MCGEN_LAUNCH_CHECK("sgd"); return 0;
}

extern "C" int mcgen_rmsprop(float* p, const float* g, float* square_avg, float* buf, int64_t n, float lr, const float* lr_dev,
                             float alpha, float eps, float momentum, float weight_decay, int64_t* step, void* stream) {
    MCGEN_CHECK(p && g && square_avg && step && n > 0, "rmsprop: bad arguments (step: int64[2] = {counter, ticket = 0})");
    MCGEN_CHECK(momentum >= 0.f && (buf != nullptr) == (momentum != 0.f), "rmsprop: buf goes with momentum > 0 (NULL when momentum = 0)");
    const size_t nv = optim_vectors(n, p, g, square_avg, buf);
    const dim3 grid(optim_grid((size_t)n, nv)), block(OPT_BLOCK);
    if (buf) hipLaunchKernelGGL(rmsprop_kernel<true>, grid, block, 0, STREAM(stream), p, g, square_avg, buf, (size_t)n, nv, lr, lr_dev, alpha, eps, momentum, weight_decay, step);
    else hipLaunchKernelGGL(rmsprop_kernel<false>, grid, block, 0, STREAM(stream), p, g, square_avg, buf, (size_t)n, nv, lr, lr_dev, alpha, eps, momentum, weight_decay, step);
    MCGEN_LAUNCH_CHECK("rmsprop"); return 0;
}

extern "C" int mcgen_adamax(float* p, const float* g, float* m, float* u, int64_t n, float lr, const float* lr_dev, float beta1,
                            float beta2, float eps, float weight_decay, int64_t* step, void* stream) {
    MCGEN_CHECK(p && g && m && u && step && n > 0, "adamax: bad arguments (step: int64[2] = {counter, ticket = 0})");
    const size_t nv = optim_vectors(n, p, g, m, u);
    hipLaunchKernelGGL(adamax_kernel, dim3(optim_grid((size_t)n, nv)), dim3(OPT_BLOCK), 0, STREAM(stream), p, g, m, u, (size_t)n, nv,
                       lr, lr_dev, beta1, beta2, eps, weight_decay, step);
    MCGEN_LAUNCH_CHECK("adamax"); return 0;
}
