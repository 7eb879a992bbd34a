// k_gradctl.hip -- the control record of sparta_grad_stats / sparta_grad_ctl_finish (include/sparta_amd.h): global-norm gradient clipping and loss scaling
// with skip-on-overflow, decided on the device.  R = kGradCtlBytes of caller-owned device memory on an 8-byte boundary: 16 words of record, then the
// partials of the reduction (one {fp64 sum of squares, int64 count} per workgroup of the largest grid).  Three kernels, none with "vbs_adam_", "vbs_sgd_" or
// "vbs_update_" in its name (the tests count the kernels of the steps by those):
//   vbs_gradctl_stats_kernel    the streaming pass over G: per workgroup the sum of the exact fp64 squares of its finite elements and the number of its
//                               Inf / NaN elements, to its slot of the partials
//   vbs_gradctl_fold_kernel     one workgroup behind it: the partials summed in slot order into words 0..2 (overwritten or added to)
//   vbs_gradctl_finish_kernel   one wave, one lane at work: words 0..5 -> norm, coef, skip, the loss scale and its growth tracker moved
// The grid of the first kernel and the slot a workgroup writes are functions of n alone, every sum runs in a fixed order and no floating-point atomic is
// used: for the same n and the same alignment of G modulo 16 bytes (the head decides which accumulator an element lands in) the record is bit-identical from
// run to run, on every device, eager or replayed.  A second launch rather than a last-workgroup-done ticket: the
// ticket needs a counter zeroed per call and a release / acquire pair per workgroup to save one launch boundary of a pass that the steps wait for anyway.
// The element kernels of k_update.hip read words 7 (coef) and 8 (skip).
#include "vbs_kernel_common.hpp"

namespace sparta_dev {
namespace {

struct GcPartial { double ssq; long long bad; };
static_assert(sizeof(GcPartial) == 16 && 64 + kGradCtlMaxGrid * sizeof(GcPartial) == kGradCtlBytes, "the partials fill R behind the record");

// one element: a finite x adds its exact square (24 x 24 bits fit the 53 of a double), anything else counts
__device__ __forceinline__ void gc_fold(float x, double& ssq, long long& bad) {
    const bool nonfinite = (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
    const double d = nonfinite ? 0.0 : (double)x;
    ssq = fma(d, d, ssq);                      // d * d is exact, so the FMA rounds once exactly where multiply-then-add would
    bad += nonfinite ? 1 : 0;
}

// {ssq, bad} of the workgroup in thread 0: lanes by xor-shuffle (64 lanes: 6 steps), then the waves in wave order
__device__ __forceinline__ void gc_block_sum(double& ssq, long long& bad) {
    __shared__ double s_ssq[kThreads / 64];
    __shared__ long long s_bad[kThreads / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ssq += __shfl_xor(ssq, o); bad += __shfl_xor(bad, o); }
    if ((threadIdx.x & 63) == 0) { s_ssq[threadIdx.x >> 6] = ssq; s_bad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ssq = s_ssq[0]; bad = s_bad[0];
#pragma unroll
        for (int wv = 1; wv < kThreads / 64; wv++) { ssq += s_ssq[wv]; bad += s_bad[wv]; }
    }
}

// G may start on any 4-byte boundary: `head` (0..3) elements one by one up to the first 16-byte boundary, n4 aligned 16-byte loads, the last
// n - head - 4 n4 one by one.  The 16-byte loads go in chunks of kThreads * kGradCtlUnroll, dealt to the workgroups round-robin: every load of a whole chunk is
// in range, so the kGradCtlUnroll loads of a lane are issued together, unguarded; the last, partial chunk is walked one load at a time by the workgroup
// whose turn it is.  Workgroup 0 takes head and tail.
__global__ __launch_bounds__(kThreads) void vbs_gradctl_stats_kernel(const float* __restrict__ G, int64_t n, int head, GcPartial* __restrict__ part) {
    constexpr int64_t kChunk = (int64_t)kThreads * kGradCtlUnroll;
    const float* body = G + head;
    const int64_t n4 = (n - head) >> 2, whole = n4 / kChunk;
    double ssq[kGradCtlUnroll];
    long long bad = 0;
#pragma unroll
    for (int u = 0; u < kGradCtlUnroll; u++) ssq[u] = 0.0;
    for (int64_t c = blockIdx.x; c < whole; c += gridDim.x) {
        const float* p = body + 4 * (c * kChunk + threadIdx.x);
        f32x4 x[kGradCtlUnroll];
#pragma unroll
        for (int u = 0; u < kGradCtlUnroll; u++) x[u] = *reinterpret_cast<const f32x4*>(p + 4 * u * kThreads);
#pragma unroll
        for (int u = 0; u < kGradCtlUnroll; u++)
#pragma unroll
            for (int e = 0; e < 4; e++) gc_fold(x[u][e], ssq[u], bad);
    }
    if ((int64_t)blockIdx.x == whole % gridDim.x) {
        for (int64_t i = whole * kChunk + threadIdx.x; i < n4; i += kThreads) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(body + 4 * i);
#pragma unroll
            for (int e = 0; e < 4; e++) gc_fold(x[e], ssq[0], bad);
        }
    }
    if (blockIdx.x == 0) {
        if ((int)threadIdx.x < head) gc_fold(G[threadIdx.x], ssq[0], bad);
        const int64_t t = head + 4 * n4 + threadIdx.x;
        if (t < n) gc_fold(G[t], ssq[0], bad);
    }
    double s = ssq[0];
#pragma unroll
    for (int u = 1; u < kGradCtlUnroll; u++) s += ssq[u];
    gc_block_sum(s, bad);
    if (threadIdx.x == 0) part[blockIdx.x] = GcPartial{s, bad};
}

// thread t sums the slots t, t + 256, ... in that order; then the workgroup's sum.  The count saturates at 2^31 - 1.
__global__ __launch_bounds__(kThreads) void vbs_gradctl_fold_kernel(uint32_t* R, int n_part, int accumulate) {
    const GcPartial* part = reinterpret_cast<const GcPartial*>(R + 16);
    double ssq = 0.0;
    long long bad = 0;
    for (int i = threadIdx.x; i < n_part; i += kThreads) { ssq += part[i].ssq; bad += part[i].bad; }
    gc_block_sum(ssq, bad);
    if (threadIdx.x != 0) return;
    if (accumulate) { ssq = *reinterpret_cast<const double*>(R) + ssq; bad += (long long)(int32_t)R[2]; }
    *reinterpret_cast<double*>(R) = ssq;
    R[2] = (uint32_t)(bad > 0x7fffffffLL ? 0x7fffffffLL : bad);
    R[3] = 0u;
}

// The arithmetic include/sparta_amd.h pins: every fp32 operation rounded once, never contracted; division and square root correctly rounded (no fast-math
// flag on this file).
__global__ __launch_bounds__(64) void vbs_gradctl_finish_kernel(uint32_t* R, float max_norm, float growth_factor, float backoff_factor, int32_t growth_interval) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    const double ssq = *reinterpret_cast<const double*>(R);
    float s = R[4] == 0u ? 1.0f : __uint_as_float(R[4]);
    int32_t tracker = (int32_t)R[5];
    const float inv = 1.0f / s;
    bool bad = (int32_t)R[2] != 0;
    const float root = (float)sqrt(ssq);
    const float norm = root * inv;
    if (!isfinite(norm)) bad = true;
    float coef = inv;
    if (!bad && max_norm > 0.0f) {
        const float c = max_norm / (norm + 1e-6f);
        if (c < 1.0f) coef = inv * c;
    }
    if (bad) coef = 0.0f;
    if (growth_interval > 0) {
        if (bad) { s = s * backoff_factor; tracker = 0; }
        else {
            tracker += 1;
            if (tracker >= growth_interval) {
                const float s2 = s * growth_factor;
                if (isfinite(s2)) s = s2;
                tracker = 0;
            }
        }
    }
    R[4] = __float_as_uint(s); R[5] = (uint32_t)tracker; R[6] = __float_as_uint(norm); R[7] = __float_as_uint(coef);
    R[8] = bad ? 1u : 0u; R[9] = R[9] + (bad ? 1u : 0u);
#pragma unroll
    for (int i = 10; i < 16; i++) R[i] = 0u;
}

}  // namespace

// the grid: one workgroup per chunk of kGradCtlChunk elements of n, at most kGradCtlMaxGrid -- a function of n alone (not of the device, not of where G starts)
unsigned grad_stats_grid(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kGradCtlChunk - 1) / kGradCtlChunk, kGradCtlMaxGrid));
}

void launch_grad_stats(hipStream_t st, const float* G, int64_t n, void* R, bool accumulate) {
    int n_part = 0;
    if (n > 0) {
        const int head = (int)std::min<int64_t>(n, (int64_t)((16 - ((uintptr_t)G & 15)) & 15) / 4);
        n_part = (int)grad_stats_grid(n);
        hipLaunchKernelGGL(vbs_gradctl_stats_kernel, dim3(n_part), dim3(kThreads), 0, st, G, n, head, reinterpret_cast<GcPartial*>((uint32_t*)R + 16));
    } else if (accumulate) {
        return;                                 // nothing to add
    }
    hipLaunchKernelGGL(vbs_gradctl_fold_kernel, dim3(1), dim3(kThreads), 0, st, (uint32_t*)R, n_part, accumulate ? 1 : 0);
}

void launch_grad_ctl_finish(hipStream_t st, void* R, float max_norm, float growth_factor, float backoff_factor, int32_t growth_interval) {
    hipLaunchKernelGGL(vbs_gradctl_finish_kernel, dim3(1), dim3(64), 0, st, (uint32_t*)R, max_norm, growth_factor, backoff_factor, growth_interval);
}

}  // namespace sparta_dev
