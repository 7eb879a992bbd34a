// k_update.hip -- sparta_vbs_set_values: new values (nztot floats in the mab layout: column-major h x w blocks back to back) written into
// the device images of a handle made with SPARTA_CREATE_UPDATABLE, without touching its plans.  Three kernels, all memory-bound:
//   vbs_update_copy_kernel      the reference-layout image of an fp32 handle (d_A is mab itself)
//   vbs_update_f32_frag_kernel  the fragment image of the fp32 one-tile plan (k_f32_direct.hip), k-compaction redone per step
//   vbs_update_h16_kernel       the 16-bit slices of the stream plans and of the hub plan (k_h16.hip, k_hub16.hip)
//   vbs_spmm_t_image_kernel     the 16-bit image of the transposed product (k_spmm_t.hip), handles made with SPARTA_CREATE_TRANSPOSE as well
// Every kernel writes exactly the elements creation wrote (the slices behind the end of an image keep what creation left there) and reads mab
// only where the plan says a stored element is: nothing is read past mab + nztot.  Offsets are 64-bit throughout.
#include "vbs_kernel_common.hpp"

namespace sparta_dev {
namespace {

constexpr int kUpdMaxGrid = 65536;      // grid cap, as launch_f32_legacy_from_frag

__global__ __launch_bounds__(kThreads) void vbs_update_copy_kernel(const float* __restrict__ mab, int64_t n, float* __restrict__ A) {
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride)      // (the caller's array may start on any 4-byte boundary)
        *reinterpret_cast<f32x4*>(A + 4 * i) = *reinterpret_cast<const f32x4u*>(mab + 4 * i);
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) A[i] = mab[i];
}

// The forward of vbs_f32_legacy_from_frag_kernel.  One wave per step q of the one-tile plan (four steps per workgroup and pass): lane = (row m = lane & 31,
// half g = lane >> 5).  Load i (0..15) of a lane reads element (m, k = 2 i + g) of the step's slice -- the 32 lanes of a half read 32 consecutive floats of
// one column -- and its ballot gives the "column has a non-zero in the tile's rows" bits of the columns 2 i and 2 i + 1; rows >= mt belong to the next tile of
// the block-row (or to nobody) and are neither read nor counted.  The position table follows from the 32 bits by the rule the host packer uses
// (frag_position).  The values go through a 4 KB image in LDS, [position][row], and leave it as the slice wants them: 16-byte quads [row][e = 0..3] of one
// (j, g), 1 KB of consecutive addresses per store instruction.  Empty columns and rows >= mt are stored as zeros (their loads were masked to zero).
__global__ __launch_bounds__(kThreads) void vbs_update_f32_frag_kernel(StepRec* steps, int64_t n_steps, const float* __restrict__ mab, float* __restrict__ a_frag,
                                                                       float* __restrict__ A_out) {
    __shared__ float img[kThreads / 64][32 * 32];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 31, g = lane >> 5;
    float* im = img[wave];
    for (int64_t q0 = (int64_t)blockIdx.x * (kThreads / 64); q0 < n_steps; q0 += (int64_t)gridDim.x * (kThreads / 64)) {
        const int64_t q = q0 + wave;
        const bool active = q < n_steps;                        // wave-uniform
        int64_t a_off = 0, h = 0;
        int mt = 0;
        if (active) { a_off = steps[q].a_off; h = steps[q].h; mt = steps[q].mt_flags & 0xffff; }
        float v[16];
        uint32_t nonempty = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int k = 2 * i + g;
            v[i] = m < mt ? mab[a_off + (int64_t)k * h + m] : 0.0f;
            const unsigned long long b = __ballot(v[i] != 0.0f);
            nonempty |= ((uint32_t)b != 0u ? 1u : 0u) << (2 * i) | ((uint32_t)(b >> 32) != 0u ? 1u : 0u) << (2 * i + 1);
        }
        if (active && A_out != nullptr && m < mt) {
#pragma unroll
            for (int i = 0; i < 16; i++) A_out[a_off + (int64_t)(2 * i + g) * h + m] = v[i];
        }
#pragma unroll
        for (int i = 0; i < 16; i++) im[frag_position(nonempty, 2 * i + g) * 32 + m] = v[i];
        __syncthreads();
        if (active) {
            float* sl = a_frag + q * kAFragSlice;
            if (lane < 8) {                                     // the table: 32 bytes in front of the slice
                uint32_t t4 = 0;
#pragma unroll
                for (int e = 0; e < 4; e++) t4 |= (uint32_t)frag_position(nonempty, 4 * lane + e) << (8 * e);
                reinterpret_cast<uint32_t*>(sl)[lane] = t4;
            }
            if (lane == 0) steps[q].mt_flags = (steps[q].mt_flags & ~(7 << STEP_KPAIRS_SHIFT)) | ((frag_pairs(nonempty) - 1) << STEP_KPAIRS_SHIFT);
            float* frag = sl + 16;
#pragma unroll
            for (int t = 0; t < 4; t++) {                       // fragment position 16 gg + 4 j + e at frag[((j * 2 + gg) * 32 + row) * 4 + e]
                const int jg = 2 * t + g, j = jg >> 1, gg = jg & 1, p0 = 16 * gg + 4 * j;
                f32x4 o;
                o[0] = im[(p0 + 0) * 32 + m]; o[1] = im[(p0 + 1) * 32 + m]; o[2] = im[(p0 + 2) * 32 + m]; o[3] = im[(p0 + 3) * 32 + m];
                *reinterpret_cast<f32x4*>(frag + (jg * 32 + m) * 4) = o;
            }
        }
        __syncthreads();
    }
}

// fp32 -> fp16 / bf16 bits exactly as to_h16 (vbs_plan.cpp) rounds at creation: round to nearest even; bf16 keeps a NaN a NaN (quiet bit set), Inf stays Inf
template <bool BF16>
__device__ __forceinline__ uint32_t upd_h16(float v) {
    if constexpr (BF16) {
        const uint32_t u = __float_as_uint(v);
        if ((u & 0x7fffffffu) > 0x7f800000u) return ((u >> 16) | 0x40u) & 0xffffu;
        return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    } else {
        const _Float16 hh = (_Float16)v;
        return (uint32_t)__builtin_bit_cast(uint16_t, hh);
    }
}

// One lane = one 16-byte chunk of one slice: 8 consecutive k of one row.  Chunk c of a slice is (k chunk kc = c / TMS, row rr = c % TMS): neighbouring lanes
// hold neighbouring rows, so each of the 8 loads of a wave reads runs of consecutive floats of one column.  Stream slices store chunk c at c (the layout
// [k / 8][row][8]: consecutive lanes, consecutive chunks); hub slices at the swizzled place of k_hub16.hip's LDS image.  Rows the map does not cover are zeros.
template <bool BF16, bool HUB, int TMS, int KP>
__global__ __launch_bounds__(kThreads) void vbs_update_h16_kernel(const UpdSlice* __restrict__ map, int64_t n_slices, const float* __restrict__ mab, uint16_t* __restrict__ dst) {
    constexpr int kChunks = TMS * KP / 8;
    const int64_t total = n_slices * kChunks, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x; id < total; id += stride) {
        const int64_t s = id / kChunks;
        const int c = (int)(id % kChunks), kc = c / TMS, rr = c % TMS;
        const UpdSlice u = map[s];
        const float* src = nullptr;
        int64_t ld = 0;
        if (rr < u.rows_lo) { src = mab + u.off_lo + rr; ld = u.h_lo; }
        else if (rr >= 32 && rr - 32 < u.rows_hi) { src = mab + u.off_hi + (rr - 32); ld = u.h_hi; }
        u32x4 o = {0u, 0u, 0u, 0u};
        if (src != nullptr) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; e++) x[e] = src[(int64_t)(kc * 8 + e) * ld];
#pragma unroll
            for (int e = 0; e < 4; e++) o[e] = upd_h16<BF16>(x[2 * e]) | (upd_h16<BF16>(x[2 * e + 1]) << 16);
        }
        const int at = HUB ? rr * 64 + ((kc ^ ((rr >> 1) & 7)) << 3) : c * 8;
        *reinterpret_cast<u32x4*>(dst + s * (int64_t)(TMS * KP) + at) = o;
    }
}

// The image of sparta_vbs_spmm_t: per block [ceil(h / 8)][w][8] -- chunk c = kc * w + q holds rows 8 kc .. 8 kc + 7 of stored column q (rows past h: zeros), what
// pack_spmm_t_block (vbs_plan.cpp) writes at creation.  One wave per block and pass; a lane writes one 16-byte chunk from 8 consecutive floats of one column of mab.
template <bool BF16>
__global__ __launch_bounds__(kThreads) void vbs_spmm_t_image_kernel(const SpmmTSrc* __restrict__ src, int64_t n_blocks, int w, const float* __restrict__ mab, uint16_t* __restrict__ dst) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t bi = (int64_t)blockIdx.x * (kThreads / 64) + wave; bi < n_blocks; bi += (int64_t)gridDim.x * (kThreads / 64)) {
        const SpmmTSrc s = src[bi];
        const int64_t chunks = (int64_t)((s.h + 7) / 8) * w;
        for (int64_t c = lane; c < chunks; c += 64) {
            const int64_t kc = c / w, q = c - kc * w;
            const float* sp = mab + s.src + q * s.h + kc * 8;
            const int rem = s.h - (int)(kc * 8);
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; e++) x[e] = e < rem ? sp[e] : 0.0f;
            u32x4 o;
#pragma unroll
            for (int e = 0; e < 4; e++) o[e] = upd_h16<BF16>(x[2 * e]) | (upd_h16<BF16>(x[2 * e + 1]) << 16);
            *reinterpret_cast<u32x4*>(dst + s.dst + c * 8) = o;
        }
    }
}

unsigned upd_grid(int64_t work_items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(work_items, kUpdMaxGrid)); }

template <bool BF16>
void launch_update_h16_t(bool hub, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const float* mab, uint16_t* dst) {
    const dim3 block(kThreads);
    if (hub) hipLaunchKernelGGL((vbs_update_h16_kernel<BF16, true, 64, 64>), dim3(upd_grid(n_slices * 2)), block, 0, st, map, n_slices, mab, dst);
    else if (tms == 32 && kp == 32) hipLaunchKernelGGL((vbs_update_h16_kernel<BF16, false, 32, 32>), dim3(upd_grid((n_slices + 1) / 2)), block, 0, st, map, n_slices, mab, dst);
    else if (tms == 64 && kp == 32) hipLaunchKernelGGL((vbs_update_h16_kernel<BF16, false, 64, 32>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, mab, dst);
    else if (tms == 32 && kp == 64) hipLaunchKernelGGL((vbs_update_h16_kernel<BF16, false, 32, 64>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, mab, dst);
    else hipLaunchKernelGGL((vbs_update_h16_kernel<BF16, false, 64, 64>), dim3(upd_grid(n_slices * 2)), block, 0, st, map, n_slices, mab, dst);
}

}  // namespace

void launch_update_copy(hipStream_t st, const float* mab, int64_t n, float* A) {
    if (n <= 0) return;
    hipLaunchKernelGGL(vbs_update_copy_kernel, dim3(upd_grid((n / 4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, mab, n, A);
}

void launch_update_f32_frag(hipStream_t st, StepRec* steps, int64_t n_steps, const float* mab, float* a_frag, float* A_out) {
    if (n_steps <= 0) return;
    hipLaunchKernelGGL(vbs_update_f32_frag_kernel, dim3(upd_grid((n_steps + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, st, steps, n_steps, mab, a_frag, A_out);
}

void launch_update_h16(bool bf16, bool hub, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const float* mab, uint16_t* dst) {
    if (n_slices <= 0) return;
    if (bf16) launch_update_h16_t<true>(hub, tms, kp, st, map, n_slices, mab, dst);
    else launch_update_h16_t<false>(hub, tms, kp, st, map, n_slices, mab, dst);
}

void launch_update_h16_t(bool bf16, hipStream_t st, const SpmmTSrc* src, int64_t n_blocks, int w, const float* mab, uint16_t* dst) {
    if (n_blocks <= 0) return;
    const dim3 grid(upd_grid((n_blocks + kThreads / 64 - 1) / (kThreads / 64))), block(kThreads);
    if (bf16) hipLaunchKernelGGL(vbs_spmm_t_image_kernel<true>, grid, block, 0, st, src, n_blocks, w, mab, dst);
    else hipLaunchKernelGGL(vbs_spmm_t_image_kernel<false>, grid, block, 0, st, src, n_blocks, w, mab, dst);
}

}  // namespace sparta_dev
