// The two other forms of an MCGlow flow (gfx950): the plain invertible 1x1 convolution InvConv2d (cfg glow.conv_lu = False,
// mcglow.py:58-73) and additive coupling (glow.affine = False, mcglow.py:160-163,172-174).  The affine / LU kernels
// are in glow_ops.hip and are not touched by these.
#include "mcgen_common.h"
#include <math.h>

namespace {
#define STREAM(s) reinterpret_cast<hipStream_t>(s)
inline int grid_for(size_t n, int block = 256, int cap = 4096) {
    size_t b = (n + block - 1) / block; if (b < 1) b = 1; if (b > (size_t)cap) b = cap; return (int)b;
}

// ---- InvConv2d: log|det W| and W^-1, one workgroup, C <= 64 --------------------------------------------------------
// Gauss-Jordan with partial pivoting on [B | A] = [W | I] -> [I | W^-1] in float64 (mcglow.py:69 takes slogdet of
// W.double()); log|det| = sum log|pivot|.  The pivot search is done by every thread on its own (the reads of one LDS word by
// all lanes are a broadcast): no shared scalar, so the dynamic 2 C^2 doubles are all the LDS the kernel has -- exactly
// the 64 KB a workgroup gets without raising the limit at C = 64.  Every loop runs C (or C^2 / blockDim) trips.
__device__ void invconv_plain_body(const float* __restrict__ W, int C, float* __restrict__ logabsdet, float* __restrict__ Winv) {
    extern __shared__ double shd[];
    double* B = shd; double* A = shd + C * C;
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) { B[i] = (double)W[i]; A[i] = (i / C == i % C) ? 1.0 : 0.0; }
    double lad = 0.0;
    bool singular = false;
    for (int col = 0; col < C; ++col) {
        __syncthreads();
        int piv = col; double bv = fabs(B[col * C + col]);
        for (int r = col + 1; r < C; ++r) { const double v = fabs(B[r * C + col]); if (v > bv) { bv = v; piv = r; } }
        if (!(bv > 0.0)) singular = true;                    // an exactly zero (or NaN) pivot column
        lad += log(bv);
        __syncthreads();                                     // everyone has read column col before the rows move
        if (piv != col)
            for (int c = threadIdx.x; c < C; c += blockDim.x) {
                double t = B[col * C + c]; B[col * C + c] = B[piv * C + c]; B[piv * C + c] = t;
                t = A[col * C + c]; A[col * C + c] = A[piv * C + c]; A[piv * C + c] = t;
            }
        __syncthreads();
        const double d = 1.0 / B[col * C + col];
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += blockDim.x) { B[col * C + c] *= d; A[col * C + c] *= d; }
        __syncthreads();
        for (int i = threadIdx.x; i < C * C; i += blockDim.x) {
            const int r = i / C, c = i % C;
            if (r != col) {
                const double f = B[r * C + col];             // column col is not written in this loop
                if (c != col) B[i] -= f * B[col * C + c];
                A[i] -= f * A[col * C + c];
            }
        }
        __syncthreads();
        for (int r = threadIdx.x; r < C; r += blockDim.x) if (r != col) B[r * C + col] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0) logabsdet[0] = singular ? -INFINITY : (float)lad;
    if (Winv)
        for (int i = threadIdx.x; i < C * C; i += blockDim.x) Winv[i] = singular ? NAN : (float)A[i];
}
__global__ void invconv_plain_kernel(const float* __restrict__ W, int C, float* __restrict__ logabsdet, float* __restrict__ Winv) {
    invconv_plain_body(W, C, logabsdet, Winv);
}
struct IcpJobs { mcgen_icp_t j[MCGEN_GLOW_BATCH_MAX]; };
__global__ void invconv_plain_batch_kernel(const IcpJobs jobs) {
    const mcgen_icp_t& j = jobs.j[blockIdx.x];
    invconv_plain_body(j.weight, j.C, j.logabsdet, j.weight_inv);
}

// ---- InvConv2d backward: grad = dW + ld_coef * W^-T ------------------------------------------------------------------
__device__ void invconv_plain_bwd_body(const float* __restrict__ dW, int C, int ldw, const float* __restrict__ Winv, float ld_coef,
                                       float* __restrict__ grad, int accumulate) {
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) {
        const int co = i / C, ci = i % C;
        const float g = fmaf(ld_coef, Winv[ci * C + co], dW[(size_t)co * ldw + ci]);
        grad[i] = accumulate ? grad[i] + g : g;
    }
}
__global__ void invconv_plain_bwd_kernel(const float* __restrict__ dW, int C, int ldw, const float* __restrict__ Winv, float ld_coef,
                                         float* __restrict__ grad, int accumulate) {
    invconv_plain_bwd_body(dW, C, ldw, Winv, ld_coef, grad, accumulate);
}
struct IcpbJobs { mcgen_icpb_t j[MCGEN_GLOW_BATCH_MAX]; };
__global__ void invconv_plain_bwd_batch_kernel(const IcpbJobs jobs) {
    const mcgen_icpb_t& j = jobs.j[blockIdx.x];
    invconv_plain_bwd_body(j.dW, j.C, j.ldw, j.weight_inv, j.ld_coef, j.grad, j.accumulate);
}

// ---- additive coupling: one thread per 8 channels of a pixel (Cp is a multiple of 8: 16-byte rows of x / y) ----------------
// The second half starts at channel C/2 of x and at channel 0 of h, so the h operands of one 8-channel group are read one by
// one: nothing is assumed about the alignment of x + C/2 against h.  Every thread reads the 8 elements of x it writes in y
// before it stores them: y == x is allowed.
template <typename T>
__global__ void coupling_add_kernel(const T* x, const T* __restrict__ h, T* y, size_t pixels, int C, int Cp,
                                    int Ch, float sign) {
    const int groups = Cp / 8, half = C / 2;
    const size_t total = pixels * groups;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / groups; const int c0 = (int)(i % groups) * 8;
        const typename Elem<T>::vec8 xv = Elem<T>::load8v(x + p * Cp + c0);
        if (c0 + 8 <= half) { *reinterpret_cast<typename Elem<T>::vec8*>(y + p * Cp + c0) = xv; continue; }      // bit copy
        typename Elem<T>::vec8 yv = xv;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = c0 + e;
            if (c >= C) yv[e] = Elem<T>::from_f(0.f);
            else if (c >= half) yv[e] = Elem<T>::from_f(fmaf(sign, Elem<T>::to_f(h[p * Ch + (c - half)]), Elem<T>::to_f(xv[e])));
        }
        *reinterpret_cast<typename Elem<T>::vec8*>(y + p * Cp + c0) = yv;
    }
}

template <typename J, typename F>
int variant_batches(const J* jobs, int n, F launch) {
    for (int base = 0; base < n; base += MCGEN_GLOW_BATCH_MAX) {
        const int m = n - base < MCGEN_GLOW_BATCH_MAX ? n - base : MCGEN_GLOW_BATCH_MAX;
        if (int rc = launch(jobs + base, m)) return rc;
    }
    return 0;
}
}  // namespace

extern "C" int mcgen_invconv_plain(const float* weight, int C, float* logabsdet, float* weight_inv, void* stream) {
    MCGEN_CHECK(weight && logabsdet && C > 0 && C <= 64, "invconv_plain: C must be in 1..64");
    hipLaunchKernelGGL(invconv_plain_kernel, dim3(1), dim3(256), 2 * (size_t)C * C * sizeof(double), STREAM(stream),
                       weight, C, logabsdet, weight_inv);
    MCGEN_LAUNCH_CHECK("invconv_plain"); return 0;
}

extern "C" int mcgen_invconv_plain_batch(const mcgen_icp_t* jobs, int n, void* stream) {
    MCGEN_CHECK(jobs && n > 0, "invconv_plain_batch: bad arguments");
    return variant_batches(jobs, n, [&](const mcgen_icp_t* j, int m) {
        IcpJobs t; int cmax = 1;
        for (int i = 0; i < m; ++i) {
            MCGEN_CHECK(j[i].weight && j[i].logabsdet && j[i].C > 0 && j[i].C <= 64, "invconv_plain_batch: bad job %d (C in 1..64)", i);
            t.j[i] = j[i]; if (j[i].C > cmax) cmax = j[i].C;
        }
        for (int i = m; i < MCGEN_GLOW_BATCH_MAX; ++i) t.j[i] = t.j[0];
        hipLaunchKernelGGL(invconv_plain_batch_kernel, dim3(m), dim3(256), 2 * (size_t)cmax * cmax * sizeof(double), STREAM(stream), t);
        MCGEN_LAUNCH_CHECK("invconv_plain_batch"); return 0;
    });
}

extern "C" int mcgen_invconv_plain_bwd(const float* dW, int C, int ldw, const float* weight_inv, float ld_coef, float* grad,
                                       int accumulate, void* stream) {
    MCGEN_CHECK(dW && weight_inv && grad && C > 0 && C <= 64 && ldw >= C, "invconv_plain_bwd: bad arguments (C in 1..64, ldw >= C)");
    hipLaunchKernelGGL(invconv_plain_bwd_kernel, dim3(1), dim3(256), 0, STREAM(stream), dW, C, ldw, weight_inv, ld_coef, grad, accumulate);
    MCGEN_LAUNCH_CHECK("invconv_plain_bwd"); return 0;
}

extern "C" int mcgen_invconv_plain_bwd_batch(const mcgen_icpb_t* jobs, int n, void* stream) {
    MCGEN_CHECK(jobs && n > 0, "invconv_plain_bwd_batch: bad arguments");
    return variant_batches(jobs, n, [&](const mcgen_icpb_t* j, int m) {
        IcpbJobs t;
        for (int i = 0; i < m; ++i) {
            MCGEN_CHECK(j[i].dW && j[i].weight_inv && j[i].grad && j[i].C > 0 && j[i].C <= 64 && j[i].ldw >= j[i].C,
                        "invconv_plain_bwd_batch: bad job %d", i);
            t.j[i] = j[i];
        }
        for (int i = m; i < MCGEN_GLOW_BATCH_MAX; ++i) t.j[i] = t.j[0];
        hipLaunchKernelGGL(invconv_plain_bwd_batch_kernel, dim3(m), dim3(256), 0, STREAM(stream), t);
        MCGEN_LAUNCH_CHECK("invconv_plain_bwd_batch"); return 0;
    });
}

extern "C" int mcgen_glow_coupling_add(const void* x, const void* h, void* y, int dtype, int64_t pixels, int C, int Cp, int Ch,
                                       int sign, void* stream) {
    MCGEN_CHECK(x && h && y && pixels > 0 && C > 0 && C % 2 == 0 && Cp >= C && Cp % 8 == 0 && Ch >= C / 2 && (sign == 1 || sign == -1),
                "glow_coupling_add: bad arguments (C even, Cp a multiple of 8 >= C, Ch >= C/2, sign +-1)");
    const size_t total = (size_t)pixels * (Cp / 8);
    if (dtype == MCGEN_F32)
        hipLaunchKernelGGL(coupling_add_kernel<float>, dim3(grid_for(total)), dim3(256), 0, STREAM(stream), (const float*)x,
                           (const float*)h, (float*)y, (size_t)pixels, C, Cp, Ch, (float)sign);
    else if (dtype == MCGEN_BF16)
        hipLaunchKernelGGL(coupling_add_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, STREAM(stream), (const bf16_t*)x,
                           (const bf16_t*)h, (bf16_t*)y, (size_t)pixels, C, Cp, Ch, (float)sign);
    else return mcgen_fail("unknown dtype %d", dtype);
    MCGEN_LAUNCH_CHECK("glow_coupling_add"); return 0;
}
