// k_f32_packed.hip -- the no-barrier fp32 kernel of the one-tile plan on PACKED steps: the partly empty blocks of a tile share a step.
// Part of the device side of libsparta_amd.so; see vbs_device.hpp for the translation-unit map, vbs_plan.cpp ("PACKED PLAN") for the
// host side and DESIGN.md section 3.2.
#include "vbs_kernel_common.hpp"

using namespace sparta_dev;

namespace {

// =====================================================================================================
// vbs_spmm_f32_packed_kernel: vbs_spmm_f32_direct_kernel (k_f32_direct.hip) with steps that are not blocks.
//
// A step holds up to 8 SLOTS; a slot is one aligned group of 4 columns of one stored block of the tile (= 4 consecutive rows of B), and
// MFMA pair s of the step consumes exactly slot s.  What is the same as in the direct kernel: no barrier, wave v owns columns
// [32 v, 32 v + 32), records through the v_readlane window, loads three steps ahead, scalar branches around the MFMA pairs a step does not
// have, the epilogue (accumulate, both layouts of C, c_nt, split images, the C ring).  What differs:
//   * B: lane (column c = lane >> 3 of a group of eight, slot s = lane & 7) loads the 16 bytes B[row_s .. row_s + 3][column] -- the gather
//     happens on the LOAD side.  row_s comes from the step's table (the first 32 bytes of its slice): voffset = column part + 4 row_s, ONE
//     descriptor over the slab of B (or over B_tail for the step of the zero-padded last block column).  An unused slot holds kPackNoRow:
//     its voffset lies past the end of the descriptor, the load returns zeros and touches no memory.
//   * the table of step i + 5 is requested with the A loads of step i + 3: the B loads of a step wait for a table that is two steps old,
//     like the panel they are written out behind.  Four table registers (step index mod 4).
//   * LDS: the image Bs[column][k'] is written in natural slot order with CONSTANT per-lane addresses: slot s, element e of the group at
//     k' = 16 (e >> 1) + 2 s + (e & 1), i.e. two 8-byte pieces 64 bytes apart -- one ds_write2_b64 per group of eight columns, four per
//     step (the direct kernel: 16 ds_write_b32 at addresses computed per step from its position table).  The fragment reads are the
//     direct kernel's four ds_read_b128, and the A fragments sit where pair s finds slot s (vbs_plan.cpp).
// No B value outside a stored block is ever multiplied: pairs behind the step's slots are not issued.
// =====================================================================================================
template <bool CSTAGE, bool TAIL = true>
__global__ __launch_bounds__(kThreads, 2) void vbs_spmm_f32_packed_kernel(const StreamParams p) {
    constexpr int TN = kTN, LDBW = 36;                  // Bs[column][k'], 32 k' + 4 padding: conflict-free ds_read_b128
    constexpr int WSTAGE = 32 * LDBW;                   // floats per wave and stage
    __shared__ __attribute__((aligned(16))) float lds[4 * 2 * WSTAGE + (CSTAGE ? 4 * kCRingFloats : 0)];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int lm = lane & 31, g = lane >> 5;
    const int n0 = blockIdx.y * TN;
    const int s_begin = p.worker_range[2 * blockIdx.x];
    const int n = p.worker_range[2 * blockIdx.x + 1] - s_begin;
    if (n <= 0) return;
    clock_probe(p.clk, 0);
    float* ws = p.ws + (int64_t)blockIdx.y * p.ws_slab_stride;

    const int32_t* srec = reinterpret_cast<const int32_t*>(p.steps + s_begin);
    // step records: the window of the direct kernel (one VGPR = the 8 records [4k, 4k + 8), every field one v_readlane with a constant lane)
    int vwin = srec[lane];
    int vnext = 0;
#define field(pos, f) __builtin_amdgcn_readlane(vwin, 8 * (pos) + (f))
    enum { F_AOFF_LO = 0, F_AOFF_HI = 1, F_BROW = 2, F_H = 3, F_CROW = 4, F_FLAGS = 5, F_SLOT = 6, F_SHARD = 7 };

    // per-lane constants.  B load q (0..3): column 8 q + (lane >> 3) of the wave's 32, slot lane & 7
    const int bc = lane >> 3, bs = lane & 7;
    const int64_t ld_t = (int64_t)p.w;                                            // leading dimension of B_tail (column-major, w rows)
    const uint32_t voffB = (uint32_t)(((32 * wave + bc) * p.ldb) * 4);
    const uint32_t voffBt = (uint32_t)(((n0 + 32 * wave + bc) * ld_t) * 4);
    const uint32_t qstepB = (uint32_t)(8 * p.ldb * 4), qstepBt = (uint32_t)(8 * ld_t * 4);
    const uint32_t voffA = (uint32_t)((g * 32 + lm) * 16);                        // fragments: [j][g][row][4]; j advances by 1 KB
    const uint32_t voffT = (uint32_t)(bs * 4);                                    // the lane's entry of a step's table
    const uint32_t voffC = p.c_row_major ? (uint32_t)((lm * p.ldc + 32 * wave + 4 * g) * 4) : (uint32_t)((lm + (32 * wave + 4 * g) * p.ldc) * 4);
    char* const ldsw = reinterpret_cast<char*>(lds) + wave * (2 * WSTAGE * 4);   // this wave's two stages
    const uint32_t lwB = (uint32_t)((bc * LDBW + 2 * bs) * 4);                    // write: column bc (+ 8 q), k' = 2 s, 2 s + 1 and 16 + 2 s, 16 + 2 s + 1
    const uint32_t lrB = (uint32_t)((lm * LDBW + 16 * g) * 4);                    // read: column lm, k' = 16 g + 4 j .. + 3
    // the slab of B: every valid voffset is below 2^31 (the launch code checks the leading dimension), 4 x kPackNoRow is not
    const __amdgpu_buffer_rsrc_t rBslab = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.B + (int64_t)n0 * p.ldb), 0, 0x7ffffff0, 0x00020000);

    u32x4 bs0[4], bs1[4];                                // B staging sets (steps of even / odd index)
    u32x4 as0[4], as1[4], as2[4], as3[4];                // A fragment sets (step index mod 4)
    uint32_t tb0 = 0, tb1 = 0, tb2 = 0, tb3 = 0;         // the lane's table entry of the steps (index mod 4) whose B loads are still to be issued

    const float* a_cur = p.A + (int64_t)s_begin * kAFragSlice;  // slice of the next step whose fragments are requested (steps are requested in order)
    uint32_t vo_cur = voffB;
    int32_t tail_prev = 0;
    auto load_table = [&](const float* slice, uint32_t& tb) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(slice), 0, 32, 0x00020000);
        tb = __builtin_amdgcn_raw_buffer_load_b32(rT, voffT, 0, 0);
    };
    // G(step) in two halves: the B panel (through the step's table); its A fragments + the table of the step two further on
    auto issue_loads_b = [&](auto pos_tag, u32x4 (&rb)[4], uint32_t tb) __attribute__((always_inline)) -> int32_t {
        constexpr int s = decltype(pos_tag)::value;      // position of the step's record in the window
        const int32_t flags = field(s, F_FLAGS);
        if constexpr (TAIL) {
            const int32_t tail = (flags & STEP_TAIL) != 0;
            if (tail != tail_prev) {
                vo_cur = tail ? voffBt : voffB;
                asm volatile("" : "+v"(vo_cur));
                tail_prev = tail;
            }
            const float* bptr = tail ? p.B_tail : p.B + (int64_t)n0 * p.ldb;     // (a tail step's table holds rows of B_tail)
            const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bptr), 0, 0x7ffffff0, 0x00020000);
            const uint32_t qs = tail ? qstepBt : qstepB;
            const uint32_t vo = vo_cur + (tb << 2);
#pragma unroll
            for (int q = 0; q < 4; q++) rb[q] = __builtin_amdgcn_raw_buffer_load_b128(rB, vo, qs * q, 0);
        } else {
            const uint32_t vo = voffB + (tb << 2);
#pragma unroll
            for (int q = 0; q < 4; q++) rb[q] = __builtin_amdgcn_raw_buffer_load_b128(rBslab, vo, qstepB * q, 0);
        }
        return flags;
    };
    auto issue_loads_a = [&](int32_t flags, u32x4 (&ra)[4], uint32_t& tb_new) __attribute__((always_inline)) {
        // the fragments this step's MFMAs will read: 1 KB per two slots; the groups behind are not fetched -- loads past the end of the
        // descriptor return zeros without touching memory
        const int32_t n_quads = (((flags >> STEP_KPAIRS_SHIFT) & 7) >> 1) + 1;
        const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a_cur + 16), 0, n_quads * 1024, 0x00020000);
#pragma unroll
        for (int j = 0; j < 4; j++) ra[j] = __builtin_amdgcn_raw_buffer_load_b128(rA, voffA, 1024 * j, 0);
        load_table(a_cur + 2 * kAFragSlice, tb_new);
        a_cur += kAFragSlice;
    };
    int32_t fq0 = 0, fq1 = 0, fq2 = 0, fq_new = 0;

    // the lane's 16 bytes (slot bs, elements 0..3 of the group) of column bc + 8 q: elements 0, 1 at k' = 2 s, elements 2, 3 at k' = 16 + 2 s
    auto write_b_q = [&](auto stage_tag, auto q_tag, const u32x4 (&rb)[4]) __attribute__((always_inline)) {
        constexpr int ST = decltype(stage_tag)::value, q = decltype(q_tag)::value;
        char* wp = ldsw + lwB + (ST * WSTAGE + 8 * q * LDBW) * 4;
        uint2 lo, hi;
        lo.x = rb[q][0]; lo.y = rb[q][1]; hi.x = rb[q][2]; hi.y = rb[q][3];
        *reinterpret_cast<uint2*>(wp) = lo;
        *reinterpret_cast<uint2*>(wp + 64) = hi;
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;

    CRing cr;                                            // CSTAGE: finished tiles wait here for whole aligned blocks of 32 rows (vbs_kernel_common.hpp)
    cr.ring = lds + 4 * 2 * WSTAGE + wave * kCRingFloats;

    // one step: fragments of B from LDS stage PAR, the next step's panel into the other stage, up to 16 MFMAs, then the staging set that was
    // just written out and the A set of step i - 1 are refilled with step i + 3
    auto step = [&](auto u_tag, int32_t flags, u32x4 (&wa)[4], u32x4 (&nb)[4], u32x4 (&na)[4], uint32_t tb_use, uint32_t& tb_new) __attribute__((always_inline)) {
        constexpr int i = decltype(u_tag)::value;        // step index mod 4 = position of its record in the window
        constexpr int PAR = i & 1;
        f32x4 fb[4];
#pragma unroll
        for (int j = 0; j < 4; j++) fb[j] = *reinterpret_cast<const f32x4*>(ldsw + lrB + (PAR * WSTAGE + 4 * j) * 4);
        // as in the direct kernel the step's other work sits BETWEEN its MFMA pairs: pairs 0..3 are followed by the LDS writes of one group of eight
        // columns of the NEXT step's panel, pair 4 by the B loads of step i + 3, pair 5 by its A loads and the table of step i + 5.  The pairs a step
        // does not have are skipped (scalar branches); the work between them always runs.
        const int32_t n_pairs = ((flags >> STEP_KPAIRS_SHIFT) & 7) + 1;
        int32_t flags_new = 0;
        static_for<0, 8>([&](auto t2_tag) __attribute__((always_inline)) {
            constexpr int t2 = decltype(t2_tag)::value;
            if (t2 < n_pairs) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[t2 >> 1][2 * (t2 & 1)], __uint_as_float(wa[t2 >> 1][2 * (t2 & 1)]), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[t2 >> 1][2 * (t2 & 1) + 1], __uint_as_float(wa[t2 >> 1][2 * (t2 & 1) + 1]), acc, 0, 0, 0);
            }
            if constexpr (t2 < 4) {
                write_b_q(std::integral_constant<int, 1 - PAR>{}, t2_tag, nb);
            } else if constexpr (t2 == 4) {
                flags_new = issue_loads_b(std::integral_constant<int, i + 3>{}, nb, tb_use);      // G(i + 3), B half: refills the staging set just written out
            } else if constexpr (t2 == 5) {
                issue_loads_a(flags_new, na, tb_new);                                             // G(i + 3), A half; table of step i + 5
            }
        });
        fq_new = flags_new;
        if (flags & STEP_LAST) {
            // epilogue (as in vbs_spmm_f32_direct_kernel): stored from copies, accumulators cleared here
            if (flags & STEP_SPLIT) {
                const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(ws + (int64_t)field(i, F_SLOT) * SK_SLOT_FLOATS, 0, SK_SLOT_FLOATS * 4, 0x00020000);
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc[q]), rW, (uint32_t)tid * 4u, (uint32_t)(q * kThreads * 4), 0);
                    __builtin_amdgcn_raw_buffer_store_b32(0u, rW, (uint32_t)tid * 4u, (uint32_t)((16 + q) * kThreads * 4), 0);   // rows 32..63 of the image: none
                }
            } else if (CSTAGE) {
                cr.park(p, n0, lm, g, voffC, acc, field(i, F_CROW), flags & 0xffff);
            } else {
                const int mt = flags & 0xffff;
                const int64_t c_row = field(i, F_CROW);
                float* cbase = p.c_row_major ? p.C + c_row * p.ldc + n0 : p.C + c_row + (int64_t)n0 * p.ldc;
                const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc(cbase, 0, 0x7ffffff0, 0x00020000);
                const uint32_t jstep = p.c_row_major ? 4u : (uint32_t)p.ldc * 4u;          // bytes per output column
                if (lm < mt) {
                    float v[16];
#pragma unroll
                    for (int q = 0; q < 16; q++) v[q] = acc[q];
                    if (p.accumulate) {
                        uint32_t old[16];
#pragma unroll
                        for (int q = 0; q < 16; q++) old[q] = __builtin_amdgcn_raw_buffer_load_b32(rC, voffC, (uint32_t)((q & 3) + 8 * (q >> 2)) * jstep, 0);
#pragma unroll
                        for (int q = 0; q < 16; q++) v[q] += __uint_as_float(old[q]);
                    }
                    if (p.c_nt) {
#pragma unroll
                        for (int q = 0; q < 16; q++) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q]), rC, voffC, (uint32_t)((q & 3) + 8 * (q >> 2)) * jstep, 2);
                    } else {
#pragma unroll
                        for (int q = 0; q < 16; q++) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q]), rC, voffC, (uint32_t)((q & 3) + 8 * (q >> 2)) * jstep, 0);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 16; q++) acc[q] = 0.0f;
        }
    };

    using c0 = std::integral_constant<int, 0>;
    using c1 = std::integral_constant<int, 1>;
    using c2 = std::integral_constant<int, 2>;
    using c3 = std::integral_constant<int, 3>;
    // the window of steps [i, i + 4): requested one round earlier (36 loads are issued in between: vmcnt(16) is a free wait).  Both sides
    // are inline asm on purpose, see vbs_spmm_f32_stream_kernel.
    auto window_swap = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(16)" : "+v"(vnext) : : "memory");
        vwin = vnext;
    };
    auto window_request = [&](int i) __attribute__((always_inline)) {
        const int32_t* nb = srec + (int64_t)(i + 4) * 8 + lane;
        asm volatile("global_load_dword %0, %1, off" : "=&v"(vnext) : "v"(nb) : "memory");
    };
    // prologue: tables of steps 0..2 first (their B loads need them), then G(0), G(1), W(0), G(2); G(k)'s A half requests the table of step k + 2
    load_table(a_cur, tb0);
    load_table(a_cur + kAFragSlice, tb1);
    fq0 = issue_loads_b(c0{}, bs0, tb0);
    issue_loads_a(fq0, as0, tb2);
    fq1 = issue_loads_b(c1{}, bs1, tb1);
    issue_loads_a(fq1, as1, tb3);
#pragma unroll
    for (int q = 0; q < 4; q++) {                        // W(0)
        char* wp = ldsw + lwB + (8 * q * LDBW) * 4;
        uint2 lo, hi;
        lo.x = bs0[q][0]; lo.y = bs0[q][1]; hi.x = bs0[q][2]; hi.y = bs0[q][3];
        *reinterpret_cast<uint2*>(wp) = lo;
        *reinterpret_cast<uint2*>(wp + 64) = hi;
    }
    fq2 = issue_loads_b(c2{}, bs0, tb2);
    issue_loads_a(fq2, as2, tb0);
    // step i: LDS stage i & 1, A set i & 3; writes out staging set (i + 1) & 1 and refills it, and A set (i + 3) & 3, with step i + 3 (table
    // register (i + 3) & 3); the table of step i + 5 goes to register (i + 1) & 3
    const int n4 = n & ~3;
    for (int i = 0; i < n4; i += 4) {
        if (i > 0) window_swap();
        window_request(i);
        step(c0{}, fq0, as0, bs1, as3, tb3, tb1);
        fq0 = fq1; fq1 = fq2; fq2 = fq_new;
        step(c1{}, fq0, as1, bs0, as0, tb0, tb2);
        fq0 = fq1; fq1 = fq2; fq2 = fq_new;
        step(c2{}, fq0, as2, bs1, as1, tb1, tb3);
        fq0 = fq1; fq1 = fq2; fq2 = fq_new;
        step(c3{}, fq0, as3, bs0, as2, tb2, tb0);
        fq0 = fq1; fq1 = fq2; fq2 = fq_new;
    }
    if (n > n4) {
        if (n4 > 0) window_swap();
        step(c0{}, fq0, as0, bs1, as3, tb3, tb1);
        fq0 = fq1; fq1 = fq2; fq2 = fq_new;
        if (n - n4 >= 2) {
            step(c1{}, fq0, as1, bs0, as0, tb0, tb2);
            fq0 = fq1; fq1 = fq2; fq2 = fq_new;
        }
        if (n - n4 == 3) step(c2{}, fq0, as2, bs1, as1, tb1, tb3);
    }
    if (CSTAGE) cr.flush(p, n0, lm, g, voffC, true);
    clock_probe(p.clk, 2);
#undef field
}

// The reference-layout image of A rebuilt from the packed image (see vbs_f32_legacy_from_frag_kernel, k_f32_direct.hip: same use, same contract): block q of the
// one-tile plan sits in slice loc[q].step; its non-empty groups (mask = loc[q].slot0_mask >> 8) take the slots from loc[q].slot0_mask & 255 on in ascending order, slot s /
// element e / row m at frag[((j * 2 + g) * 32 + m) * 4 + e'] with j = s >> 1, g = e >> 1, e' = 2 (s & 1) + (e & 1); empty groups are zeros.  The copy is exact.
__global__ __launch_bounds__(kThreads) void vbs_f32_legacy_from_pack_kernel(const StepRec* steps, const PackLoc* loc, int64_t n_steps, const float* a_pack, float* A) {
    for (int64_t q = blockIdx.x; q < n_steps; q += gridDim.x) {
        const int64_t a_off = steps[q].a_off, h = steps[q].h;
        const int mt = steps[q].mt_flags & 0xffff;
        const float* frag = a_pack + (int64_t)loc[q].step * kAFragSlice + 16;
        const uint32_t mask = ((uint32_t)loc[q].slot0_mask >> 8) & 0xffu, slot0 = (uint32_t)loc[q].slot0_mask & 0xffu;
        for (int x = threadIdx.x; x < 32 * 32; x += kThreads) {
            const int k = x >> 5, m = x & 31;
            if (m >= mt) continue;
            const int gm = k >> 2, e = k & 3;
            float v = 0.0f;
            if ((mask >> gm) & 1u) {
                const int s = (int)slot0 + __builtin_popcount(mask & ((1u << gm) - 1u));
                v = frag[(((s >> 1) * 2 + (e >> 1)) * 32 + m) * 4 + 2 * (s & 1) + (e & 1)];
            }
            A[a_off + (int64_t)k * h + m] = v;
        }
    }
}

}  // namespace

namespace sparta_dev {

void launch_f32_legacy_from_pack(hipStream_t st, const StepRec* steps, const PackLoc* loc, int64_t n_steps, const float* a_pack, float* A) {
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_steps, 65536));
    hipLaunchKernelGGL(vbs_f32_legacy_from_pack_kernel, dim3(grid), dim3(kThreads), 0, st, steps, loc, n_steps, a_pack, A);
}

void launch_f32_packed(bool c_stage, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (sp.B_tail != nullptr) {
        if (c_stage) hipLaunchKernelGGL((vbs_spmm_f32_packed_kernel<true, true>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_spmm_f32_packed_kernel<false, true>), grid, dim3(kThreads), 0, st, sp);
    } else {
        if (c_stage) hipLaunchKernelGGL((vbs_spmm_f32_packed_kernel<true, false>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_spmm_f32_packed_kernel<false, false>), grid, dim3(kThreads), 0, st, sp);
    }
}

}  // namespace sparta_dev
