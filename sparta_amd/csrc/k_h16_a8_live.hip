// k_h16_a8_live.hip -- the fp8 weight image with a live-block set (sparta_vbs_set_a8_live).
//   vbs_fwdq8lv_h16_kernel  the body of k_h16_direct.inc with H16_DIRECT_LIVE = 1 and H16_DIRECT_A8 = 1: it walks the compacted records and live ranges of live
//                           forward (k_live.hip) and reads the e4m3 image -- a step's slice by its own record (an element offset is a byte offset there), a dead
//                           half through the zero-record descriptor (code 0 is +0.0 under any scale) with its B fragments ANDed with 0, a wholly dead step
//                           without a panel of B, and the scales from the last word of the step's record.  The instantiations of the a8 form (k_h16_a8.hip),
//                           same template arguments: the launch code takes the 128-column sibling where the live form would take the 256-column slab or the
//                           four accumulators.  Not here: gathered B, DEEP, the LDS-staged kernel.
//   vbs_q8lv_scales_kernel  puts the exponent words where that kernel reads them: position p of the compacted records gets the last word of the private a8
//                           record of the slice its a_off names.  One thread per position, plain 4-byte vector stores, every position written on every launch;
//                           no atomics, no LDS.  Launched behind every compaction and behind every quantise launch while the switch is on.
// (The names avoid what the code-object tests of the other forms count: "vbs_fwda8_h16_kernel", "vbs_fwdlive_", "vbs_live_", "vbs_a8quant_kernel", ...)
#include "vbs_kernel_common.hpp"

using namespace sparta_dev;

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define H16_DIRECT_KERNEL vbs_fwdq8lv_h16_kernel
#define H16_DIRECT_LIVE 1
#define H16_DIRECT_A8 1
#include "k_h16_direct.inc"
#undef H16_DIRECT_KERNEL
#undef H16_DIRECT_LIVE
#undef H16_DIRECT_A8

// slice s of the image lies behind step s of the private records (ensure_a8_arrays checks a_off = base + s * slice on the plain records, of which the compacted
// array is a per-range permutation): s = (a_off - base) / slice.  A record whose offset names no slice (none exists) is left alone.
__global__ __launch_bounds__(kThreads) void vbs_q8lv_scales_kernel(const StepRec* __restrict__ a8_recs, int64_t n_steps, int64_t base, int64_t slice,
                                                                 StepRec* __restrict__ live_recs) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < n_steps; p += stride) {
        const int64_t d = live_recs[p].a_off - base, s = d / slice;
        if (d >= 0 && s < n_steps) live_recs[p].pad = a8_recs[s].pad;
    }
}

// BF16 and TAIL (some step reads the zero-padded copy of the last rows of B) from the call
template <int KP, bool MI2, bool CSTAGE, int WC>
void launch_q8lv_v(bool bf16, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (sp.B_tail != nullptr) {
        if (bf16) hipLaunchKernelGGL((vbs_fwdq8lv_h16_kernel<KP, MI2, true, false, CSTAGE, false, true, WC, false>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_fwdq8lv_h16_kernel<KP, MI2, false, false, CSTAGE, false, true, WC, false>), grid, dim3(kThreads), 0, st, sp);
    } else {
        if (bf16) hipLaunchKernelGGL((vbs_fwdq8lv_h16_kernel<KP, MI2, true, false, CSTAGE, false, false, WC, false>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_fwdq8lv_h16_kernel<KP, MI2, false, false, CSTAGE, false, false, WC, false>), grid, dim3(kThreads), 0, st, sp);
    }
}

}  // namespace

namespace sparta_dev {

// the choices of launch_h16_a8_stream (k_h16_a8.hip)
void launch_h16_a8_live_stream(int kp, bool mi2, bool bf16, bool c_stage, bool wide, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (mi2) {
        if (kp == 64) launch_q8lv_v<64, true, false, 32>(bf16, grid, st, sp);
        else launch_q8lv_v<32, true, false, 32>(bf16, grid, st, sp);
    } else if (kp == 64) {
        if (c_stage) launch_q8lv_v<64, false, true, 32>(bf16, grid, st, sp);
        else launch_q8lv_v<64, false, false, 32>(bf16, grid, st, sp);
    } else if (wide) {
        launch_q8lv_v<32, false, false, 64>(bf16, grid, st, sp);
    } else {
        if (c_stage) launch_q8lv_v<32, false, true, 32>(bf16, grid, st, sp);
        else launch_q8lv_v<32, false, false, 32>(bf16, grid, st, sp);
    }
}

// one thread per position of the compacted records, the grid cap of the word kernel
void launch_a8_live_scales(hipStream_t st, const StepRec* a8_recs, int64_t n_steps, int64_t base, int64_t slice, StepRec* live_recs) {
    if (n_steps <= 0 || slice <= 0) return;
    const int64_t groups = (n_steps + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(vbs_q8lv_scales_kernel, dim3((unsigned)std::min<int64_t>(groups, 65536)), dim3(kThreads), 0, st, a8_recs, n_steps, base, slice, live_recs);
}

}  // namespace sparta_dev
