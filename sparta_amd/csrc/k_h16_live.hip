// k_h16_live.hip -- the live form of the no-barrier 16-bit stream kernel (sparta_vbs_set_live_forward): vbs_fwdlive_h16_kernel is the
// body of k_h16_direct.inc with H16_DIRECT_LIVE = 1.  It walks the compacted records and live ranges that vbs_fwdlive_compact_kernel (k_live.hip) writes
// behind every sparta_vbs_set_live_blocks: the steps of dead blocks are not in a worker's live range, the kept ones carry their own slice offset, and the
// absent flags mark what is dead of a kept step.  A translation unit of its own: the plain instantiations of k_h16.hip do not wait for these.
// Instantiated for what a qualifying handle launches by default -- both 16-bit types, KP 32 / 64, TAIL on / off, one-tile WC 32 with and without the C ring,
// WC 64, the 256-column slab form, pair / 64-row tiles and QUAD.  Not here: gathered B, DEEP (SPARTA_H16_AHEAD=7) and the LDS-staged kernel; the launch
// code keeps the plain kernels on the plain records there (h16_live_form_available, k_h16.hip).
#include "vbs_kernel_common.hpp"

using namespace sparta_dev;

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define H16_DIRECT_KERNEL vbs_fwdlive_h16_kernel
#define H16_DIRECT_LIVE 1
#include "k_h16_direct.inc"
#undef H16_DIRECT_KERNEL
#undef H16_DIRECT_LIVE

// BF16 and TAIL (some step reads the zero-padded copy of the last rows of B) from the call
template <int KP, bool MI2, bool CSTAGE, int WC, bool SLAB>
void launch_live_v(bool bf16, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (sp.B_tail != nullptr) {
        if (bf16) hipLaunchKernelGGL((vbs_fwdlive_h16_kernel<KP, MI2, true, false, CSTAGE, false, true, WC, SLAB>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_fwdlive_h16_kernel<KP, MI2, false, false, CSTAGE, false, true, WC, SLAB>), grid, dim3(kThreads), 0, st, sp);
    } else {
        if (bf16) hipLaunchKernelGGL((vbs_fwdlive_h16_kernel<KP, MI2, true, false, CSTAGE, false, false, WC, SLAB>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_fwdlive_h16_kernel<KP, MI2, false, false, CSTAGE, false, false, WC, SLAB>), grid, dim3(kThreads), 0, st, sp);
    }
}

}  // namespace

namespace sparta_dev {

// the choices of launch_h16_stream (k_h16.hip) for a B that is not gathered and loads three steps ahead
void launch_h16_live_stream(int kp, bool mi2, bool bf16, bool c_stage, bool wide, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (mi2) {
        if (kp == 64) launch_live_v<64, true, false, 32, false>(bf16, grid, st, sp);
        else launch_live_v<32, true, false, 32, false>(bf16, grid, st, sp);
    } else if (kp == 64) {
        if (c_stage) launch_live_v<64, false, true, 32, false>(bf16, grid, st, sp);
        else launch_live_v<64, false, false, 32, false>(bf16, grid, st, sp);
    } else if (wide) {
        launch_live_v<32, false, false, 64, false>(bf16, grid, st, sp);
    } else {
        if (c_stage) launch_live_v<32, false, true, 32, false>(bf16, grid, st, sp);
        else launch_live_v<32, false, false, 32, false>(bf16, grid, st, sp);
    }
}

void launch_h16_live_slab256(bool bf16, dim3 grid, hipStream_t st, const StreamParams& sp) { launch_live_v<32, false, false, 64, true>(bf16, grid, st, sp); }

void launch_h16_live_quad(int kp, bool bf16, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (kp == 64) launch_live_v<64, true, false, 64, true>(bf16, grid, st, sp);
    else launch_live_v<32, true, false, 64, true>(bf16, grid, st, sp);
}

}  // namespace sparta_dev
