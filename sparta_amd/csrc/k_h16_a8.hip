// k_h16_a8.hip -- the fp8 weight image of 16-bit handles (sparta_vbs_set_forward_a8).
//   vbs_a8quant_kernel    a sibling of vbs_update_h16_kernel on the same UpdSlice map: one WAVE per slice gathers each of its groups (32 rows x KP values) from
//                         mab, reduces the largest finite |v| across its 64 lanes by shuffles, and writes the e4m3 codes ([k / 8][row][8], one byte each) and the
//                         biased exponents (the last word of the slice's private step record) with vector stores.  No atomics, no LDS, no dependence on the
//                         launch geometry: bit-identical from run to run, capturable.  The rule is a8_exponent / a8_code (vbs_kernel_common.hpp), which
//                         sparta_a8_quantize_group runs on the host.
//   vbs_fwda8_h16_kernel  the body of k_h16_direct.inc with H16_DIRECT_A8 = 1: 8-byte loads of codes, widened by v_cvt_scalef32_pk_{f16,bf16}_fp8 in front of
//                         the MFMAs.  Instantiated for the 128-column launches of a qualifying handle -- both 16-bit types, KP 32 / 64, TAIL on / off, one-tile
//                         WC 32 with and without the C ring, WC 64 (two sub-workers), pair / 64-row tiles.  Not here: the 256-column slab and the
//                         four-accumulator form (the launch code takes the 128-column sibling on the same records), gathered B, DEEP, the LDS-staged kernel.
#include "vbs_kernel_common.hpp"

using namespace sparta_dev;

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define H16_DIRECT_KERNEL vbs_fwda8_h16_kernel
#define H16_DIRECT_LIVE 0
#define H16_DIRECT_A8 1
#include "k_h16_direct.inc"
#undef H16_DIRECT_KERNEL
#undef H16_DIRECT_LIVE
#undef H16_DIRECT_A8

// lane = (row lm = lane & 31 of the group, g = lane >> 5): it holds the chunks kc = 2 j + g, j < KP / 16, of its row -- the 32 lanes of a half read 32
// consecutive floats of one column of mab, as the sibling's loads do, and store 256 consecutive bytes of the image.  Rows the map does not cover hold
// zeros and belong to no group; a group without rows has e = 0.
template <int TMS, int KP>
__global__ __launch_bounds__(kThreads) void vbs_a8quant_kernel(const UpdSlice* __restrict__ map, int64_t n_slices, const float* __restrict__ mab, uint8_t* __restrict__ dst,
                                                               StepRec* __restrict__ recs) {
    constexpr int NH = TMS / 32, NC = KP / 16;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lm = lane & 31, g = lane >> 5;
    for (int64_t s = (int64_t)blockIdx.x * (kThreads / 64) + wave; s < n_slices; s += (int64_t)gridDim.x * (kThreads / 64)) {      // (s: the whole wave's)
        const UpdSlice u = map[s];
        uint32_t word = 0;
#pragma unroll
        for (int hf = 0; hf < NH; hf++) {
            const int rr = 32 * hf + lm;
            const float* src = nullptr;
            int64_t ld = 0;
            if (rr < u.rows_lo) { src = mab + u.off_lo + rr; ld = u.h_lo; }
            else if (rr >= 32 && rr - 32 < u.rows_hi) { src = mab + u.off_hi + (rr - 32); ld = u.h_hi; }
            uint32_t x[NC][8];
#pragma unroll
            for (int j = 0; j < NC; j++)
#pragma unroll
                for (int e = 0; e < 8; e++) x[j][e] = 0u;
            if (src != nullptr) {
#pragma unroll
                for (int j = 0; j < NC; j++)
#pragma unroll
                    for (int e = 0; e < 8; e++) x[j][e] = __float_as_uint(src[(int64_t)((2 * j + g) * 8 + e) * ld]);
            }
            uint32_t amax = 0u;
#pragma unroll
            for (int j = 0; j < NC; j++)
#pragma unroll
                for (int e = 0; e < 8; e++) amax = a8_amax_bits(amax, x[j][e]);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)amax, off, 64);
                amax = o > amax ? o : amax;
            }
            const int32_t ex = a8_exponent(amax);
            const float inv = __uint_as_float(a8_inv_scale_bits(ex));
#pragma unroll
            for (int j = 0; j < NC; j++) {
                u32x2 o = {0u, 0u};
#pragma unroll
                for (int e = 0; e < 8; e++) o[e >> 2] |= a8_code(__float_as_uint(__uint_as_float(x[j][e]) * inv)) << (8 * (e & 3));
                *reinterpret_cast<u32x2*>(dst + s * (int64_t)(TMS * KP) + ((2 * j + g) * TMS + rr) * 8) = o;
            }
            word |= (uint32_t)(ex + 127) << (16 * hf);
        }
        if (lane == 0) recs[s].pad = (int32_t)word;
    }
}

// BF16 and TAIL (some step reads the zero-padded copy of the last rows of B) from the call
template <int KP, bool MI2, bool CSTAGE, int WC>
void launch_a8_v(bool bf16, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (sp.B_tail != nullptr) {
        if (bf16) hipLaunchKernelGGL((vbs_fwda8_h16_kernel<KP, MI2, true, false, CSTAGE, false, true, WC, false>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_fwda8_h16_kernel<KP, MI2, false, false, CSTAGE, false, true, WC, false>), grid, dim3(kThreads), 0, st, sp);
    } else {
        if (bf16) hipLaunchKernelGGL((vbs_fwda8_h16_kernel<KP, MI2, true, false, CSTAGE, false, false, WC, false>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_fwda8_h16_kernel<KP, MI2, false, false, CSTAGE, false, false, WC, false>), grid, dim3(kThreads), 0, st, sp);
    }
}

}  // namespace

namespace sparta_dev {

// the choices of launch_h16_stream (k_h16.hip) for a B that is not gathered and loads three steps ahead
void launch_h16_a8_stream(int kp, bool mi2, bool bf16, bool c_stage, bool wide, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (mi2) {
        if (kp == 64) launch_a8_v<64, true, false, 32>(bf16, grid, st, sp);
        else launch_a8_v<32, true, false, 32>(bf16, grid, st, sp);
    } else if (kp == 64) {
        if (c_stage) launch_a8_v<64, false, true, 32>(bf16, grid, st, sp);
        else launch_a8_v<64, false, false, 32>(bf16, grid, st, sp);
    } else if (wide) {
        launch_a8_v<32, false, false, 64>(bf16, grid, st, sp);
    } else {
        if (c_stage) launch_a8_v<32, false, true, 32>(bf16, grid, st, sp);
        else launch_a8_v<32, false, false, 32>(bf16, grid, st, sp);
    }
}

// one wave per slice, the grid cap of the set_values kernels
void launch_a8_quantize(int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const float* mab, uint8_t* dst, StepRec* recs) {
    if (n_slices <= 0) return;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((n_slices + kThreads / 64 - 1) / (kThreads / 64), 65536))), block(kThreads);
    if (tms == 32 && kp == 32) hipLaunchKernelGGL((vbs_a8quant_kernel<32, 32>), grid, block, 0, st, map, n_slices, mab, dst, recs);
    else if (tms == 64 && kp == 32) hipLaunchKernelGGL((vbs_a8quant_kernel<64, 32>), grid, block, 0, st, map, n_slices, mab, dst, recs);
    else if (tms == 32 && kp == 64) hipLaunchKernelGGL((vbs_a8quant_kernel<32, 64>), grid, block, 0, st, map, n_slices, mab, dst, recs);
    else hipLaunchKernelGGL((vbs_a8quant_kernel<64, 64>), grid, block, 0, st, map, n_slices, mab, dst, recs);
}

}  // namespace sparta_dev
