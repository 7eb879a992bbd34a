// k_prune.hip -- block pruning on the stored blocks of a VBS handle (sparta_vbs_block_ssq / sparta_vbs_mask_blocks, include/sparta_amd.h).  Both kernels walk the
// block table (PruneBlock, vbs_device.hpp: offset, n_in, n_all per stored block in mab order) and touch nothing of the handle's images: W and T0..T3 are the
// caller's tensors in the mab layout.  Neither name holds "vbs_adam_", "vbs_sgd_" or "vbs_update_" (the tests count the kernels of the steps by those):
//   vbs_prune_block_ssq_kernel   per block the fp64 sum of the exact squares of its first n_in elements (the ones inside the matrix)
//   vbs_prune_mask_kernel        the blocks with keep[b] == 0 stored as +0.0f, all n_all elements, in up to four tensors; the other blocks are not touched
// One WAVE per block, kPruneWaves blocks per workgroup, and a block is never split between waves: a score is a function of the block's own elements and of
// where it starts modulo 16 bytes alone -- not of its neighbours, of the grid or of the device -- with no cross-wave step, no LDS and no barrier, and a kept
// block costs the mask kernel one byte read.  Blocks of a trained layer are a few thousand elements (a 64 x 64 block is 16 loads of 16 bytes per lane); a
// 266 x 200 block next to 1 x 1 blocks leaves the other waves of its workgroup idle while one wave streams 208 KB, which the other workgroups of the grid
// cover.  Both kernels are bandwidth-bound streams: 16-byte accesses wherever the block allows them, the loads of the sum four deep per lane.
#include "vbs_kernel_common.hpp"

namespace sparta_dev {
namespace {

// plain IEEE: an Inf or a NaN inside the matrix makes the score non-finite.  x * x is exact in fp64 (24 x 24 bits), so the FMA rounds once, where the add would
__device__ __forceinline__ void pr_fold(float x, double& ssq) {
    const double d = (double)x;
    ssq = fma(d, d, ssq);
}

// elements up to the first 16-byte boundary of a run of n floats at p (blocks start anywhere: offsets are arbitrary and so is the tensor's base)
__device__ __forceinline__ int pr_head(const float* p, int n) {
    const int to_boundary = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    return n < to_boundary ? n : to_boundary;
}

// The lane's elements in a fixed order: 16-byte loads lane, lane + 64, ... of the aligned body (four in flight per lane, each to its own accumulator; the
// remainder one at a time into the first), then the head element and the tail element into the first; accumulators summed 0..3; lanes by xor-shuffle.
__global__ __launch_bounds__(kThreads) void vbs_prune_block_ssq_kernel(const PruneBlock* __restrict__ blocks, int64_t n_blocks, const float* __restrict__ W,
                                                                      double* __restrict__ ssq_out) {
    const int64_t b = (int64_t)blockIdx.x * kPruneWaves + (threadIdx.x >> 6);
    if (b >= n_blocks) return;                  // (the whole wave)
    const int lane = threadIdx.x & 63;
    const PruneBlock blk = blocks[b];
    const float* p = W + blk.off;
    const int n = blk.n_in;
    const int head = pr_head(p, n);
    const float* body = p + head;
    const int n4 = (n - head) >> 2;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int i = lane;
    for (; i + 192 < n4; i += 256) {
        f32x4 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = *reinterpret_cast<const f32x4*>(body + 4 * (i + 64 * u));
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int e = 0; e < 4; e++) pr_fold(x[u][e], acc[u]);
    }
    for (; i < n4; i += 64) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(body + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; e++) pr_fold(x[e], acc[0]);
    }
    if (lane < head) pr_fold(p[lane], acc[0]);
    const int t = head + 4 * n4 + lane;
    if (t < n) pr_fold(p[t], acc[0]);
    double s = ((acc[0] + acc[1]) + acc[2]) + acc[3];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) ssq_out[b] = s;
}

// n floats at p stored as +0.0f by one wave: head, aligned 16-byte stores, tail.  Nothing is read.
__device__ __forceinline__ void pr_zero_run(float* p, int n, int lane) {
    const int head = pr_head(p, n);
    float* body = p + head;
    const int n4 = (n - head) >> 2;
    if (lane < head) p[lane] = 0.0f;
    for (int i = lane; i < n4; i += 64) *reinterpret_cast<f32x4*>(body + 4 * i) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int t = head + 4 * n4 + lane;
    if (t < n) p[t] = 0.0f;
}

__global__ __launch_bounds__(kThreads) void vbs_prune_mask_kernel(const PruneBlock* __restrict__ blocks, int64_t n_blocks, const uint8_t* __restrict__ keep, float* T0,
                                                                 float* T1, float* T2, float* T3) {
    const int64_t b = (int64_t)blockIdx.x * kPruneWaves + (threadIdx.x >> 6);
    if (b >= n_blocks || keep[b] != 0) return;  // (the whole wave: a kept block is neither read nor written)
    const int lane = threadIdx.x & 63;
    const PruneBlock blk = blocks[b];
    if (T0) pr_zero_run(T0 + blk.off, blk.n_all, lane);
    if (T1) pr_zero_run(T1 + blk.off, blk.n_all, lane);
    if (T2) pr_zero_run(T2 + blk.off, blk.n_all, lane);
    if (T3) pr_zero_run(T3 + blk.off, blk.n_all, lane);
}

unsigned prune_grid(int64_t n_blocks) { return (unsigned)((n_blocks + kPruneWaves - 1) / kPruneWaves); }

}  // namespace

void launch_block_ssq(hipStream_t st, const PruneBlock* blocks, int64_t n_blocks, const float* W, double* ssq) {
    hipLaunchKernelGGL(vbs_prune_block_ssq_kernel, dim3(prune_grid(n_blocks)), dim3(kThreads), 0, st, blocks, n_blocks, W, ssq);
}

void launch_mask_blocks(hipStream_t st, const PruneBlock* blocks, int64_t n_blocks, const uint8_t* keep, float* T0, float* T1, float* T2, float* T3) {
    hipLaunchKernelGGL(vbs_prune_mask_kernel, dim3(prune_grid(n_blocks)), dim3(kThreads), 0, st, blocks, n_blocks, keep, T0, T1, T2, T3);
}

}  // namespace sparta_dev
