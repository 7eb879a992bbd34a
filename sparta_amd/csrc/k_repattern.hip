// k_repattern.hip -- the values and the optimizer state of a layer moved from the mab layout of one VBS handle to that of another (sparta_vbs_move_blocks,
// include/sparta_amd.h).  One kernel, whose name holds none of the strings the tests count kernels by ("vbs_prune_", "vbs_adam_", "vbs_sgd_", "vbs_update_",
// "stream_kernel", "direct_kernel", "sddmm", "gradctl", ...):
//   vbs_repat_move_kernel   per destination block the n_all elements of its source block copied bit for bit, or n_all stores of +0.0f for a new block, in
//                           up to four tensor pairs
// The scheme of k_prune.hip: one WAVE per destination block, kPruneWaves blocks per workgroup, a block never split between waves, no LDS, no atomics, no
// cross-wave step.  A block's record (MoveBlock, vbs_device.hpp) is read once and serves all four pairs.  The stores are laid out on the DESTINATION's 16-byte
// grid as pr_zero_run lays them out: a head up to the first 16-byte boundary, 16-byte stores, a tail.  Where the source run starts at the same offset modulo
// 16 bytes (a compaction keeps most runs so: blocks are multiples of 16 bytes whenever h * w % 4 == 0) the body is read by 16-byte loads, four in flight per
// lane; elsewhere by 4-byte loads, eight in flight per lane (two destination vectors) -- a misaligned vector pointer is never dereferenced.  The words travel
// as uint32: no float instruction sees a payload.  A bandwidth-bound stream: the blocks of a trained layer are a few thousand elements each.
#include "vbs_kernel_common.hpp"

namespace sparta_dev {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// elements up to the first 16-byte boundary of a run of n words at p
__device__ __forceinline__ int rp_head(const uint32_t* p, int n) {
    const int to_boundary = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    return n < to_boundary ? n : to_boundary;
}

// n words from s to d by one wave
__device__ __forceinline__ void rp_copy_run(const uint32_t* __restrict__ s, uint32_t* __restrict__ d, int n, int lane) {
    const int head = rp_head(d, n);
    uint32_t* body = d + head;
    const uint32_t* sbody = s + head;
    const int n4 = (n - head) >> 2;
    if (lane < head) d[lane] = s[lane];
    int i = lane;
    if (((uintptr_t)sbody & 15u) == 0) {                                                  // (the whole wave: s and d are the block's)
        for (; i + 192 < n4; i += 256) {
            u32x4 x[4];
#pragma unroll
            for (int u = 0; u < 4; u++) x[u] = *reinterpret_cast<const u32x4*>(sbody + 4 * (i + 64 * u));
#pragma unroll
            for (int u = 0; u < 4; u++) *reinterpret_cast<u32x4*>(body + 4 * (i + 64 * u)) = x[u];
        }
        for (; i < n4; i += 64) *reinterpret_cast<u32x4*>(body + 4 * i) = *reinterpret_cast<const u32x4*>(sbody + 4 * i);
    } else {
        for (; i + 64 < n4; i += 128) {
            uint32_t x[2][4];
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int e = 0; e < 4; e++) x[u][e] = sbody[4 * (i + 64 * u) + e];
#pragma unroll
            for (int u = 0; u < 2; u++) *reinterpret_cast<u32x4*>(body + 4 * (i + 64 * u)) = u32x4{x[u][0], x[u][1], x[u][2], x[u][3]};
        }
        for (; i < n4; i += 64) {
            uint32_t x[4];
#pragma unroll
            for (int e = 0; e < 4; e++) x[e] = sbody[4 * i + e];
            *reinterpret_cast<u32x4*>(body + 4 * i) = u32x4{x[0], x[1], x[2], x[3]};
        }
    }
    const int t = head + 4 * n4 + lane;
    if (t < n) d[t] = s[t];
}

// n words at d stored as 0 (+0.0f) by one wave; nothing is read
__device__ __forceinline__ void rp_zero_run(uint32_t* d, int n, int lane) {
    const int head = rp_head(d, n);
    uint32_t* body = d + head;
    const int n4 = (n - head) >> 2;
    if (lane < head) d[lane] = 0u;
    for (int i = lane; i < n4; i += 64) *reinterpret_cast<u32x4*>(body + 4 * i) = u32x4{0u, 0u, 0u, 0u};
    const int t = head + 4 * n4 + lane;
    if (t < n) d[t] = 0u;
}

__device__ __forceinline__ void rp_pair(const MoveBlock& blk, const uint32_t* S, uint32_t* D, int lane) {
    if (!D) return;
    if (blk.moved) rp_copy_run(S + blk.src_off, D + blk.dst_off, blk.n_all, lane);
    else rp_zero_run(D + blk.dst_off, blk.n_all, lane);
}

__global__ __launch_bounds__(kThreads) void vbs_repat_move_kernel(const MoveBlock* __restrict__ blocks, int64_t n_blocks, const uint32_t* S0, uint32_t* D0,
                                                                 const uint32_t* S1, uint32_t* D1, const uint32_t* S2, uint32_t* D2, const uint32_t* S3,
                                                                 uint32_t* D3) {
    const int64_t b = (int64_t)blockIdx.x * kPruneWaves + (threadIdx.x >> 6);
    if (b >= n_blocks) return;                  // (the whole wave)
    const int lane = threadIdx.x & 63;
    const MoveBlock blk = blocks[b];
    rp_pair(blk, S0, D0, lane);
    rp_pair(blk, S1, D1, lane);
    rp_pair(blk, S2, D2, lane);
    rp_pair(blk, S3, D3, lane);
}

}  // namespace

void launch_move_blocks(hipStream_t st, const MoveBlock* blocks, int64_t n_blocks, const float* const* S, float* const* D) {
    const unsigned grid = (unsigned)((n_blocks + kPruneWaves - 1) / kPruneWaves);
    const uint32_t* s[4];
    uint32_t* d[4];
    for (int q = 0; q < 4; q++) {
        s[q] = reinterpret_cast<const uint32_t*>(S[q]);
        d[q] = reinterpret_cast<uint32_t*>(D[q]);
    }
    hipLaunchKernelGGL(vbs_repat_move_kernel, dim3(grid), dim3(kThreads), 0, st, blocks, n_blocks, s[0], d[0], s[1], d[1], s[2], d[2], s[3], d[3]);
}

}  // namespace sparta_dev
