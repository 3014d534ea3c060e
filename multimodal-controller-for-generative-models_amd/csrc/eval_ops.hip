// Per-batch evaluation metrics summed on the device (gfx950): what compat/metrics computes with one torch pass and one host
// synchronisation per metric -- MSE / BCE / PSNR of an image pair, the cross-entropy of a logit map, top-1 accuracy, a loss
// scalar -- as reductions (one pass over the inputs; the cross-entropy reads its logits twice, maximum then exp sum) whose only result is a float64 written into two small caller-owned arrays:
//   last[slot] = the batch value v,   acc[slot] += n * v   (n = the batch size; slot -1 = not wanted)
// Inputs are read as fp32 and widened; all arithmetic, log / exp included, is fp64.  Every reduction has a fixed order and no
// atomics: a thread sums its elements serially in ascending order, a wave adds its 64 lanes with a shuffle tree, thread 0 adds
// the four waves in order through LDS and stores the workgroup's partial; a second, one-workgroup launch adds the partials in
// ascending workgroup order and finishes the value.  The grid is a function of the element count alone, so a repeated call
// returns the same bits.
//   eval_img_kernel       sum (o - t)^2 and sum of BCE terms over both tensors      (16-byte loads, grid-stride over 4-element chunks)
//   eval_nll_kernel       sum of -log softmax(logits)[target]                       (one thread per (n, pixel), lanes along the pixels)
//   eval_accuracy_kernel  hits: first argmax == label                               (one wave per row, lanes along the classes)
//   eval_*_final_kernel   partials -> value -> last / acc                           (one workgroup)
// Entry points documented in include/mcgen_hip.h.
#include "mcgen_common.h"

namespace {
#define STREAM(s) reinterpret_cast<hipStream_t>(s)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGroups = MCGEN_EVAL_GROUPS;     // most workgroups of a first pass = partials per value in `work`
constexpr int kImgSlice = 4096;                // elements per workgroup before the grid stops growing: 4 chunks a thread

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));     // a 4-float load from a 4-byte aligned address

static int groups_for(int64_t items, int per_group) {
    const int64_t g = (items + per_group - 1) / per_group;
    return (int)(g < kGroups ? g : kGroups);
}

// the workgroup's sum of v in a fixed order (lanes by a shuffle tree, then the waves ascending); every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                           // `red` may still be read from a previous call
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r += red[w];
    return r;
}

// log clamped from below at -100 as F.binary_cross_entropy does; a NaN stays a NaN
__device__ __forceinline__ double log_clamped(double x) {
    const double l = log(x);
    return l < -100.0 ? -100.0 : l;
}

__device__ __forceinline__ void img_terms(float o, float t, double& sq, double& bce) {
    const double d = (double)o - (double)t;
    sq += d * d;
    const double om = (double)((o + 1.0f) / 2.0f), tm = (double)((t + 1.0f) / 2.0f);      // the map itself is fp32 (metrics.py:24-25)
    bce -= tm * log_clamped(om) + (1.0 - tm) * log_clamped(1.0 - om);
}

// grid G <= kGroups, 256 threads: chunk c = elements 4c .. 4c + 3; thread (g, t) takes chunks g * 256 + t, + G * 256, ...
// work[g][0] = sum of squared differences, work[g][1] = sum of BCE terms
template <bool kAligned>
__global__ __launch_bounds__(kThreads) void eval_img_kernel(const float* __restrict__ out, const float* __restrict__ tgt, int64_t E,
                                                            double* __restrict__ work) {
    __shared__ double red[kWaves];
    const int64_t full = E / 4;                                       // chunks with all four elements
    const int64_t step = (int64_t)gridDim.x * kThreads;
    double sq = 0.0, bce = 0.0;
    int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
#pragma unroll 4
    for (; c < full; c += step) {
        f32x4 o, t;
        if (kAligned) {
            o = *reinterpret_cast<const f32x4*>(out + 4 * c);
            t = *reinterpret_cast<const f32x4*>(tgt + 4 * c);
        } else {
            o = *reinterpret_cast<const f32x4_a4*>(out + 4 * c);
            t = *reinterpret_cast<const f32x4_a4*>(tgt + 4 * c);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) img_terms(o[i], t[i], sq, bce);
    }
    if (c == full)                                                    // the one thread whose next chunk is the ragged tail
        for (int64_t e = 4 * full; e < E; ++e) img_terms(out[e], tgt[e], sq, bce);
    const double s0 = block_sum(sq, red), s1 = block_sum(bce, red);
    if (threadIdx.x == 0) { work[2 * blockIdx.x] = s0; work[2 * blockIdx.x + 1] = s1; }
}

// the partials of value j, j < nv, added in ascending workgroup order by thread j; sums[j] valid for every thread afterwards
__device__ __forceinline__ void sum_partials(const double* __restrict__ work, int G, int nv, double* stage, double* sums) {
    for (int i = threadIdx.x; i < G * nv; i += kThreads) stage[i] = work[i];
    __syncthreads();
    if ((int)threadIdx.x < nv) {
        double s = stage[threadIdx.x];
        for (int g = 1; g < G; ++g) s += stage[g * nv + threadIdx.x];
        sums[threadIdx.x] = s;
    }
    __syncthreads();
}

__device__ __forceinline__ void publish(int slot, double v, double n, double* acc, double* last) {
    if (slot < 0) return;
    last[slot] = v;
    acc[slot] += n * v;
}

__global__ __launch_bounds__(kThreads) void eval_img_final_kernel(const double* __restrict__ work, int G, double E, double n,
                                                                  int slot_mse, int slot_bce, int slot_psnr,
                                                                  double* __restrict__ acc, double* __restrict__ last) {
    __shared__ double stage[2 * kGroups], sums[2];
    sum_partials(work, G, 2, stage, sums);
    if (threadIdx.x != 0) return;
    const double mse = sums[0] / E;
    publish(slot_mse, mse, n, acc, last);
    publish(slot_bce, sums[1] / E, n, acc, last);
    publish(slot_psnr, 20.0 * log10(1.0 / sqrt(mse)), n, acc, last);             // compat/metrics.PSNR, max_value 1
}

// grid G <= kGroups, 256 threads over the P = N * HW positions: position p = (n, hw) reads logits[n][k][hw], k = 0 .. K - 1,
// so a wave reads 64 adjacent floats per k.  A target outside [0, K) gives NaN and reads no logit.
__global__ __launch_bounds__(kThreads) void eval_nll_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                            int64_t P, int K, int64_t HW, double* __restrict__ work) {
    __shared__ double red[kWaves];
    const int64_t step = (int64_t)gridDim.x * kThreads;
    double sum = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < P; p += step) {
        const int64_t t = target[p];
        if (t < 0 || t >= K) { sum += __builtin_nan(""); continue; }
        const float* x = logits + (p / HW) * K * HW + p % HW;
        float m = x[0];
        const float* q = x;
#pragma unroll 4
        for (int k = 1; k < K; ++k) { q += HW; m = fmaxf(m, *q); }
        bool bad = false;                                              // fmaxf drops a NaN: look for one in the second pass
        const double md = (double)m;
        double z = 0.0;
        q = x;
#pragma unroll 4
        for (int k = 0; k < K; ++k, q += HW) {
            const float v = *q;
            bad |= v != v;
            z += exp((double)v - md);
        }
        const double term = log(z) + md - (double)x[t * HW];
        sum += bad ? __builtin_nan("") : term;
    }
    const double s = block_sum(sum, red);
    if (threadIdx.x == 0) work[blockIdx.x] = s;
}

// the mean over `count` terms, or 100 * hits / count for the accuracy
__global__ __launch_bounds__(kThreads) void eval_mean_final_kernel(const double* __restrict__ work, int G, double scale, double count,
                                                                   double n, int slot, double* __restrict__ acc,
                                                                   double* __restrict__ last) {
    __shared__ double stage[kGroups], sums[1];
    sum_partials(work, G, 1, stage, sums);
    if (threadIdx.x == 0) publish(slot, scale * sums[0] / count, n, acc, last);
}

// grid G <= kGroups, 256 threads = 4 waves, a wave per row (rows g * 4 + w, + G * 4, ...): a lane keeps the first maximum of
// its classes lane, lane + 64, ..., the wave keeps the larger value and on ties the lower index.  A row with a NaN is a miss;
// a label outside [0, C) gives NaN and the row is not read.
__global__ __launch_bounds__(kThreads) void eval_accuracy_kernel(const float* __restrict__ logits, const int64_t* __restrict__ label,
                                                                 int64_t N, int C, double* __restrict__ work) {
    __shared__ double red[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double hits = 0.0;                                                 // counted in lane 0 of each wave
    for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < N; r += (int64_t)gridDim.x * kWaves) {
        const int64_t want = label[r];
        if (want < 0 || want >= C) { if (lane == 0) hits += __builtin_nan(""); continue; }
        const float* x = logits + r * C;
        float best = -__builtin_inff();
        int at = C;                                                    // no class yet: loses every tie
        int bad = 0;
        for (int c = lane; c < C; c += 64) {
            const float v = x[c];
            bad |= v != v;
            if (v > best || at == C) { if (v == v) { best = v; at = c; } }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_down(best, off);
            const int oa = __shfl_down(at, off);
            bad |= __shfl_down(bad, off);
            if (oa < C && (at == C || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
        }
        if (lane == 0 && !bad && at == (int)want) hits += 1.0;
    }
    const double s = block_sum(hits, red);
    if (threadIdx.x == 0) work[blockIdx.x] = s;
}

__global__ void eval_scalar_kernel(const float* __restrict__ value, double n, int slot, double* __restrict__ acc,
                                   double* __restrict__ last) {
    if (threadIdx.x == 0 && blockIdx.x == 0) publish(slot, (double)value[0], n, acc, last);
}

bool slot_ok(int s) { return s >= -1 && s < MCGEN_EVAL_SLOTS; }
}  // namespace

extern "C" int mcgen_eval_img(const float* out, const float* tgt, int64_t E, int64_t n, double* work, int slot_mse, int slot_bce,
                              int slot_psnr, double* acc, double* last, void* stream) {
    MCGEN_CHECK(out && tgt && work && acc && last && E > 0 && n > 0, "eval_img: bad arguments");
    MCGEN_CHECK(slot_ok(slot_mse) && slot_ok(slot_bce) && slot_ok(slot_psnr), "eval_img: a slot outside [-1, %d)", MCGEN_EVAL_SLOTS);
    MCGEN_CHECK((slot_mse < 0 || (slot_mse != slot_bce && slot_mse != slot_psnr)) && (slot_bce < 0 || slot_bce != slot_psnr),
                "eval_img: two metrics share a slot");
    MCGEN_CHECK((((uintptr_t)out | (uintptr_t)tgt) & 3) == 0, "eval_img: tensors must be 4-byte aligned");
    const int G = groups_for(E, kImgSlice);
    if ((((uintptr_t)out | (uintptr_t)tgt) & 15) == 0)
        hipLaunchKernelGGL(eval_img_kernel<true>, dim3(G), dim3(kThreads), 0, STREAM(stream), out, tgt, E, work);
    else
        hipLaunchKernelGGL(eval_img_kernel<false>, dim3(G), dim3(kThreads), 0, STREAM(stream), out, tgt, E, work);
    MCGEN_LAUNCH_CHECK("eval_img");
    hipLaunchKernelGGL(eval_img_final_kernel, dim3(1), dim3(kThreads), 0, STREAM(stream), work, G, (double)E, (double)n, slot_mse,
                       slot_bce, slot_psnr, acc, last);
    MCGEN_LAUNCH_CHECK("eval_img_final"); return 0;
}

extern "C" int mcgen_eval_nll(const float* logits, const int64_t* target, int64_t N, int K, int64_t HW, int64_t n, double* work,
                              int slot, double* acc, double* last, void* stream) {
    MCGEN_CHECK(logits && target && work && acc && last && N > 0 && N < (1ll << 31) && K > 0 && HW > 0 && HW < (1ll << 31) && n > 0,
                "eval_nll: bad arguments");
    MCGEN_CHECK(slot_ok(slot), "eval_nll: a slot outside [-1, %d)", MCGEN_EVAL_SLOTS);
    const int64_t P = N * HW;
    const int G = groups_for(P, kThreads);
    hipLaunchKernelGGL(eval_nll_kernel, dim3(G), dim3(kThreads), 0, STREAM(stream), logits, target, P, K, HW, work);
    MCGEN_LAUNCH_CHECK("eval_nll");
    hipLaunchKernelGGL(eval_mean_final_kernel, dim3(1), dim3(kThreads), 0, STREAM(stream), work, G, 1.0, (double)P, (double)n, slot,
                       acc, last);
    MCGEN_LAUNCH_CHECK("eval_nll_final"); return 0;
}

extern "C" int mcgen_eval_accuracy(const float* logits, const int64_t* label, int64_t N, int C, int64_t n, double* work, int slot,
                                   double* acc, double* last, void* stream) {
    MCGEN_CHECK(logits && label && work && acc && last && N > 0 && C > 0 && n > 0, "eval_accuracy: bad arguments");
    MCGEN_CHECK(slot_ok(slot), "eval_accuracy: a slot outside [-1, %d)", MCGEN_EVAL_SLOTS);
    const int G = groups_for(N, kWaves);
    hipLaunchKernelGGL(eval_accuracy_kernel, dim3(G), dim3(kThreads), 0, STREAM(stream), logits, label, N, C, work);
    MCGEN_LAUNCH_CHECK("eval_accuracy");
    hipLaunchKernelGGL(eval_mean_final_kernel, dim3(1), dim3(kThreads), 0, STREAM(stream), work, G, 100.0, (double)N, (double)n, slot,
                       acc, last);
    MCGEN_LAUNCH_CHECK("eval_accuracy_final"); return 0;
}

extern "C" int mcgen_eval_scalar(const float* value, int64_t n, int slot, double* acc, double* last, void* stream) {
    MCGEN_CHECK(value && acc && last && n > 0, "eval_scalar: bad arguments");
    MCGEN_CHECK(slot_ok(slot), "eval_scalar: a slot outside [-1, %d)", MCGEN_EVAL_SLOTS);
    hipLaunchKernelGGL(eval_scalar_kernel, dim3(1), dim3(64), 0, STREAM(stream), value, (double)n, slot, acc, last);
    MCGEN_LAUNCH_CHECK("eval_scalar"); return 0;
}
