// k_h16.hip -- fp16 / bf16 storage with fp32 accumulation: the LDS-staged and the direct (operands straight into the MFMA
// registers) persistent stream kernels, the 16-bit B-tail copy and the fp32 -> 16-bit conversion of the host-pointer path.
// Part of the device side of libsparta_amd.so; see vbs_device.hpp for the translation-unit map and DESIGN.md section 8.
#include "vbs_kernel_common.hpp"

using namespace sparta_dev;

namespace {

// =====================================================================================================
// 16-bit (fp16 / bf16) storage, fp32 accumulation: vbs_spmm_h16_stream_kernel<KP, MI2, BF16>
// Same persistent design, step records, plans and epilogue as the fp32 stream kernel; what changes is the operand path.
// * A is re-laid-out ONCE at sparta_vbs_create: every step's slice is a dense TM x KP chunk stored [k chunk of 8][row][8] (rows
//   past the tile zero) -- the order in which the direct kernel's lanes want it: lane (row, g) takes k chunk 2 q + g, so a wave
//   load is contiguous -- the chunks of a tile back to back.  The 16-bit MFMA wants 8 consecutive k of one row per lane; the
//   reference's column-major blocks have k strided, and transposing 16-bit data on the way into LDS costs 8 ds_write_b16 per
//   16-byte load.  The host-side VBS (the boundary) keeps the reference's layout; only the device copy differs.
// * B must be column-major (k contiguous per column) with an even leading dimension: Bs[j][k], As[i][k], rows padded by
//   8 elements; a fragment is one ds_read_b128 (8 k) per operand and feeds v_mfma_f32_32x32x16_{f16,bf16}.
// * D = Bpanel^T . Atile^T as in the fp32 kernels (accumulator layout and epilogue are the same); an MFMA sums its k slots,
//   so any lane -> k assignment works as long as both operands use the same one (lane group g takes k = kb + 8g .. +7).
// A step moves half the bytes of the fp32 kernel and its MFMAs take 1/8 of the time: this kernel is bound by the load path
// (L2 / Infinity Cache -> LDS), not by MFMA.
// =====================================================================================================
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// DEEP: four register sets instead of two -- loads run 5 steps ahead of the MFMAs (4 steps of panels in flight per workgroup
// instead of 2).  A 16-bit step has 64-128 cycles of MFMA per wave: what a step costs is how long its panel takes to arrive
// divided by the number of panels in flight, and the registers are there (2 waves per SIMD: 256 VGPRs each).
template <int KP, bool MI2, bool BF16, bool GATHERED, bool DEEP>
__global__ __launch_bounds__(kThreads, 2) void vbs_spmm_h16_stream_kernel(const StreamParams p) {
    constexpr int TN = kTN, TM = MI2 ? 64 : 32;
    constexpr int LDK = KP + 8;                          // elements per LDS row
    constexpr int BSZ = TN * LDK;                        // elements of the B panel image
    constexpr int STAGE = BSZ + 64 * LDK;                // elements per LDS stage
    constexpr int CPC = KP / 8;                          // 16-byte chunks per row / column
    constexpr int CPP = kThreads / CPC;                  // B columns covered by one load pass
    constexpr int NBL = TN / CPP;                        // B loads per thread and step (4 for KP 64, 2 for KP 32)
    constexpr int NAL = (TM * CPC + kThreads - 1) / kThreads;   // A loads per thread and step (2, 1, 1, 1)
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int lm = lane & 31, g = lane >> 5;
    const int n0 = blockIdx.y * TN;
    const int s_begin = p.worker_range[2 * blockIdx.x];
    const int n = p.worker_range[2 * blockIdx.x + 1] - s_begin;
    if (n <= 0) return;
    clock_probe(p.clk, 0);
#ifdef SPARTA_TIMELINE
    long long tl_t0 = 0;
    if (p.clk != nullptr && blockIdx.y == 0 && tid == 0 && blockIdx.x < 1024) tl_t0 = wall_clock64();
#endif
    float* ws = p.ws + (int64_t)blockIdx.y * p.ws_slab_stride;
    const uint16_t* A16 = reinterpret_cast<const uint16_t*>(p.A);
    const uint16_t* B16 = reinterpret_cast<const uint16_t*>(p.B);
    const uint16_t* Bt16 = reinterpret_cast<const uint16_t*>(p.B_tail);

    const int32_t* srec = reinterpret_cast<const int32_t*>(p.steps + s_begin);
    int vrec0 = srec[lane];
    int vrec1 = srec[64 + lane];
    int vnext = 0;
    // a macro over a free function, not a lambda: every closure between the loop body and vrec0 / vrec1 is one more level of
    // pointer indirection the optimiser has to peel before it can keep them in registers (three levels deep it gave up and
    // left one of them in memory: an LDS / scratch read behind a full wait in every step)
#define field(s, f) sk_field(vrec0, vrec1, (s), (f))
    enum { F_AOFF_LO = 0, F_AOFF_HI = 1, F_BROW = 2, F_H = 3, F_CROW = 4, F_FLAGS = 5, F_SLOT = 6, F_SHARD = 7 };

    const int bj0 = tid / CPC, bc = tid % CPC;           // B: column bj0 + CPP q, chunk bc (k = 8 bc .. 8 bc + 7)
    const int ac = tid % (TM * CPC);                     // A: 16-byte chunk ac (+ 256 q) of the contiguous slice (clamped: duplicates are harmless)
    const int64_t ld_t = (int64_t)p.w;                   // leading dimension of B_tail
    const uint32_t voffB = (uint32_t)((bc * 8 + bj0 * p.ldb) * 2), voffBt = (uint32_t)((bc * 8 + (n0 + bj0) * ld_t) * 2);
    const uint32_t qstepB = (uint32_t)(CPP * p.ldb * 2), qstepBt = (uint32_t)(CPP * ld_t * 2);
    const int64_t n0off = (int64_t)n0 * p.ldb;
    const uint32_t lwB = (uint32_t)((bj0 * LDK + bc * 8) * 2);
    const uint32_t lwA = (uint32_t)((BSZ + (ac % TM) * LDK + (ac / TM) * 8) * 2);   // slice in memory: [k chunk][row][8] (chunk ac = row ac % TM, k chunk ac / TM)
    const uint32_t lrB = (uint32_t)(((32 * wave + lm) * LDK + 8 * g) * 2);
    const uint32_t lrA = (uint32_t)((BSZ + lm * LDK + 8 * g) * 2);
    const uint32_t voffC = p.c_row_major ? (uint32_t)((lm * p.ldc + 32 * wave + 4 * g) * 4) : (uint32_t)((lm + (32 * wave + 4 * g) * p.ldc) * 4);
    char* const ldsb = reinterpret_cast<char*>(lds);

    u32x4 b0[NBL], a0[NAL], b1[NBL], a1[NAL];
    u32x4 b2[DEEP ? NBL : 1], a2[DEEP ? NAL : 1], b3[DEEP ? NBL : 1], a3[DEEP ? NAL : 1];     // DEEP: register sets 2 / 3
    constexpr int AHEAD = DEEP ? 5 : 3;                  // a register set written to LDS at step i is refilled with step i + AHEAD

    int64_t g_aoff = 0;
    uint32_t vo_cur = voffB;                             // see the fp32 kernel: every VALU instruction in the steady state costs an MFMA slot
    int32_t tail_prev = 0;
    auto issue_loads = [&](int s, u32x4 (&rb)[NBL], u32x4 (&ra)[NAL]) __attribute__((always_inline)) -> int32_t {
        const int32_t flags = field(s, F_FLAGS);
        if (flags & STEP_FIRST) g_aoff = (int64_t)(uint32_t)field(s, F_AOFF_LO) | ((int64_t)field(s, F_AOFF_HI) << 32);
        else g_aoff += (int64_t)TM * KP;                 // the slices of a tile are back to back
        const int32_t tail = (flags & STEP_TAIL) != 0;
        if (tail != tail_prev) {
            vo_cur = tail ? voffBt : voffB;
            asm volatile("" : "+v"(vo_cur));
            tail_prev = tail;
        }
        const int64_t gk0 = field(s, F_BROW);
        const uint16_t* bptr = tail ? Bt16 + gk0 : B16 + (GATHERED ? (int64_t)field(s, F_SHARD) * p.shard_stride : (int64_t)0) + gk0 + n0off;   // gathered: (slab, row inside the slab), see the fp32 kernel
        const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(bptr), 0, 0x7ffffff0, 0x00020000);
        const uint32_t qs = tail ? qstepBt : qstepB;
#pragma unroll
        for (int q = 0; q < NBL; q++) rb[q] = __builtin_amdgcn_raw_buffer_load_b128(rB, vo_cur, qs * q, 0);
        const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(A16 + g_aoff), 0, 0x7ffffff0, 0x00020000);
#pragma unroll
        for (int q = 0; q < NAL; q++) ra[q] = __builtin_amdgcn_raw_buffer_load_b128(rA, (uint32_t)ac * 16u, (uint32_t)(q * kThreads * 16), 2);
        return flags;
    };
    int32_t fq0 = 0, fq1 = 0, fq2 = 0, fq_new = 0;
    auto write_stage = [&](auto stage_tag, const u32x4 (&rb)[NBL], const u32x4 (&ra)[NAL]) __attribute__((always_inline)) {
        constexpr int ST = decltype(stage_tag)::value;
#pragma unroll
        for (int q = 0; q < NBL; q++) *reinterpret_cast<u32x4*>(ldsb + lwB + (ST * STAGE + q * CPP * LDK) * 2) = rb[q];
#pragma unroll
        for (int q = 0; q < NAL; q++) *reinterpret_cast<u32x4*>(ldsb + lwA + (ST * STAGE + q * (kThreads / TM) * 8) * 2) = ra[q];
    };

    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
    auto mfma = [&](const u32x4& bf, const u32x4& af, f32x16& acc) __attribute__((always_inline)) {
        if constexpr (BF16) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, bf), __builtin_bit_cast(bf16x8, af), acc, 0, 0, 0);
        else acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bf), __builtin_bit_cast(f16x8, af), acc, 0, 0, 0);
    };

    auto iteration_t = [&](int i, int32_t flags, u32x4 (&wb)[NBL], u32x4 (&wa)[NAL], auto par_tag) __attribute__((always_inline)) {
        constexpr int PAR = decltype(par_tag)::value;
        using nxt_t = std::integral_constant<int, 1 - PAR>;
#ifdef SPARTA_TIMELINE
        unsigned long long tl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const bool tl_on = p.clk != nullptr && blockIdx.x == 8 && blockIdx.y == 0 && i >= TL_FIRST && i < TL_FIRST + TL_STEPS;
#endif
        TL_STAMP(0);
        write_stage(nxt_t{}, wb, wa);
        TL_STAMP(1);
        fq_new = issue_loads(i + AHEAD, wb, wa);
        TL_STAMP(2);
        // pair tiles (vbs_plan.cpp): the half whose block-row has no block in this step's column is zeros in the slice; it must not meet the panel of B either
        // (0 x Inf = NaN): its B fragment is ANDed with a wave-uniform 0, see vbs_spmm_h16_direct_kernel
        const uint32_t m_lo = (MI2 && (flags & STEP_LO_ABSENT)) ? 0u : ~0u, m_hi = (MI2 && (flags & STEP_HI_ABSENT)) ? 0u : ~0u;
#pragma unroll
        for (int kb = 0; kb < KP; kb += 16) {
            const u32x4 bf = *reinterpret_cast<const u32x4*>(ldsb + lrB + (PAR * STAGE + kb) * 2);
            const u32x4 af0 = *reinterpret_cast<const u32x4*>(ldsb + lrA + (PAR * STAGE + kb) * 2);
            if constexpr (MI2) {
                const u32x4 af1 = *reinterpret_cast<const u32x4*>(ldsb + lrA + (PAR * STAGE + 32 * LDK + kb) * 2);
                mfma(u32x4{bf[0] & m_lo, bf[1] & m_lo, bf[2] & m_lo, bf[3] & m_lo}, af0, acc0);
                mfma(u32x4{bf[0] & m_hi, bf[1] & m_hi, bf[2] & m_hi, bf[3] & m_hi}, af1, acc1);
            } else {
                mfma(bf, af0, acc0);
            }
        }
        TL_STAMP(3);
        TL_STAMP(4);
        if (flags & STEP_LAST) {
            if (flags & STEP_SPLIT) {
                const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(ws + (int64_t)field(i, F_SLOT) * SK_SLOT_FLOATS, 0, SK_SLOT_FLOATS * 4, 0x00020000);
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc0[q]), rW, (uint32_t)tid * 4u, (uint32_t)(q * kThreads * 4), 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc1[q]), rW, (uint32_t)tid * 4u, (uint32_t)((16 + q) * kThreads * 4), 0);
                }
            } else {
                const int mt = flags & 0xffff;
                const int64_t c_row = field(i, F_CROW);
                float* cbase = p.c_row_major ? p.C + c_row * p.ldc + n0 : p.C + c_row + (int64_t)n0 * p.ldc;
                const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc(cbase, 0, 0x7ffffff0, 0x00020000);
                const uint32_t jstep = p.c_row_major ? 4u : (uint32_t)p.ldc * 4u;
                const uint32_t mistep = p.c_row_major ? (uint32_t)p.ldc * 128u : 128u;
#pragma unroll
                for (int mi = 0; mi < (MI2 ? 2 : 1); mi++) {
                    if (mi * 32 + lm < mt) {
                        float v[16];
#pragma unroll
                        for (int q = 0; q < 16; q++) v[q] = mi == 0 ? acc0[q] : acc1[q];
                        if (p.accumulate) {
                            uint32_t old[16];
#pragma unroll
                            for (int q = 0; q < 16; q++) old[q] = __builtin_amdgcn_raw_buffer_load_b32(rC, voffC, (uint32_t)((q & 3) + 8 * (q >> 2)) * jstep + (uint32_t)mi * mistep, 0);
#pragma unroll
                            for (int q = 0; q < 16; q++) v[q] += __uint_as_float(old[q]);
                        }
                        if (p.c_nt) {
#pragma unroll
                            for (int q = 0; q < 16; q++) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q]), rC, voffC, (uint32_t)((q & 3) + 8 * (q >> 2)) * jstep + (uint32_t)mi * mistep, 2);
                        } else {
#pragma unroll
                            for (int q = 0; q < 16; q++) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q]), rC, voffC, (uint32_t)((q & 3) + 8 * (q >> 2)) * jstep + (uint32_t)mi * mistep, 0);
                        }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 16; q++) { acc0[q] = 0.0f; acc1[q] = 0.0f; }
        }
        TL_STAMP(5);
        __syncthreads();
        TL_STAMP(6);
#ifdef SPARTA_TIMELINE
        if (tl_on) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) {
                long long* o = p.clk + 16 + ((int64_t)wave * TL_STEPS + (i - TL_FIRST)) * 8;
#pragma unroll
                for (int k = 0; k < 7; k++) o[k] = (long long)tl[k];
                o[7] = flags;
            }
        }
#endif
    };

    using st0 = std::integral_constant<int, 0>;
    using st1 = std::integral_constant<int, 1>;
    if constexpr (!DEEP) {
        fq0 = issue_loads(0, b0, a0);
        fq1 = issue_loads(1, b1, a1);
        write_stage(st0{}, b0, a0);
        fq2 = issue_loads(2, b0, a0);
        __syncthreads();
        // record batches: see the fp32 kernel.  At least 4 steps x (NBL + NAL >= 3) = 12 loads are issued between request and touch.
        auto batch_upkeep = [&](int i) __attribute__((always_inline)) {
            if ((i & 7) == 0 && i > 0) {
                const int32_t* nb = srec + (int64_t)((i >> 3) + 1) * 64 + lane;
                asm volatile("global_load_dword %0, %1, off" : "=&v"(vnext) : "v"(nb) : "memory");
            }
            if ((i & 7) == 4 && i > 4) {
                asm volatile("s_waitcnt vmcnt(3)" : "+v"(vnext) : : "memory");
                // two selects, not "if (odd) vrec1 = vnext; else vrec0 = vnext;": the compiler merges the two stores of that form into one store
                // through a selected POINTER, which pins vrec0 / vrec1 in scratch memory -- every step then reloads them behind vmcnt(0)
                const bool odd = (((i >> 3) + 1) & 1) != 0;
                vrec1 = odd ? vnext : vrec1;
                vrec0 = odd ? vrec0 : vnext;
            }
        };
        const int n_even = n & ~1;
        for (int i = 0; i < n_even; i += 2) {
            batch_upkeep(i);
            iteration_t(i, fq0, b1, a1, st0{});
            fq0 = fq1; fq1 = fq2; fq2 = fq_new;
            iteration_t(i + 1, fq0, b0, a0, st1{});
            fq0 = fq1; fq1 = fq2; fq2 = fq_new;
        }
        if (n & 1) {
            batch_upkeep(n_even);
            iteration_t(n_even, fq0, b1, a1, st0{});
        }
    } else {
        // Step s lives in register set s & 3 and LDS stage s & 1.  Iteration i computes step i, writes step i + 1 (set (i + 1) & 3)
        // into the other stage and refills that set with step i + 5: steps i + 2 .. i + 5 are in flight under step i.
        int32_t fq3 = 0, fq4 = 0;
        fq0 = issue_loads(0, b0, a0);
        fq1 = issue_loads(1, b1, a1);
        write_stage(st0{}, b0, a0);
        fq2 = issue_loads(2, b2, a2);
        fq3 = issue_loads(3, b3, a3);
        fq4 = issue_loads(4, b0, a0);
        __syncthreads();
        // Record batches (8 steps each; vrec0 / vrec1 hold batches k, k + 1): step 8k + 3 is the first to look into batch k + 1
        // (its refill is step 8k + 8), so batch k + 1 is requested at step 8k - 2 and touched at step 8k + 2; the register it
        // replaces (batch k - 1) is dead from step 8k on.  The four steps in between issue 4 x (NBL + NAL >= 3) >= 12 loads and
        // memory returns in order: vmcnt(12) at the touch is a wait the pipeline has already paid.
        auto upkeep_request = [&](int i) __attribute__((always_inline)) {
            if ((i & 7) == 6) {
                const int32_t* nb = srec + (int64_t)((i >> 3) + 2) * 64 + lane;
                asm volatile("global_load_dword %0, %1, off" : "=&v"(vnext) : "v"(nb) : "memory");
            }
        };
        auto upkeep_touch = [&](int i) __attribute__((always_inline)) {
            if ((i & 7) == 2 && i > 2) {
                asm volatile("s_waitcnt vmcnt(12)" : "+v"(vnext) : : "memory");
                // two selects, not "if (odd) vrec1 = vnext; else vrec0 = vnext;": the compiler merges the two stores of that form into one store
                // through a selected POINTER, which pins vrec0 / vrec1 in scratch memory -- every step then reloads them behind vmcnt(0)
                const bool odd = (((i >> 3) + 1) & 1) != 0;
                vrec1 = odd ? vnext : vrec1;
                vrec0 = odd ? vrec0 : vnext;
            }
        };
        auto rotate = [&]() __attribute__((always_inline)) { fq0 = fq1; fq1 = fq2; fq2 = fq3; fq3 = fq4; fq4 = fq_new; };
        const int n4 = n & ~3;
        for (int i = 0; i < n4; i += 4) {
            iteration_t(i, fq0, b1, a1, st0{});
            rotate();
            iteration_t(i + 1, fq0, b2, a2, st1{});
            rotate();
            upkeep_request(i + 2);
            upkeep_touch(i + 2);
            iteration_t(i + 2, fq0, b3, a3, st0{});
            rotate();
            iteration_t(i + 3, fq0, b0, a0, st1{});
            rotate();
        }
        // the last n & 3 steps, peeled (see the fp32 kernel on why not a break inside the loop)
        if (n & 3) {
            iteration_t(n4, fq0, b1, a1, st0{});
            rotate();
            if ((n & 3) > 1) {
                iteration_t(n4 + 1, fq0, b2, a2, st1{});
                rotate();
                if ((n & 3) > 2) {
                    upkeep_touch(n4 + 2);
                    iteration_t(n4 + 2, fq0, b3, a3, st0{});
                }
            }
        }
    }
    clock_probe(p.clk, 2);
#ifdef SPARTA_TIMELINE
    if (p.clk != nullptr && blockIdx.y == 0 && tid == 0 && blockIdx.x < 1024) {
        p.clk[16 + 4 * 64 * 8 + 2 * blockIdx.x] = tl_t0;
        p.clk[16 + 4 * 64 * 8 + 2 * blockIdx.x + 1] = wall_clock64();
    }
#endif
}

#undef field

// =====================================================================================================
// 16-bit storage without a workgroup-wide stage: vbs_spmm_h16_direct_kernel<KP, MI2, BF16, GATHERED>
// A 16-bit step has 64-256 cycles of MFMA per wave; in the LDS-staged kernel above what a step costs is its bookkeeping: the
// register -> LDS -> register round trip of BOTH operands, one workgroup barrier and the four waves waiting for each other
// (measured with the in-kernel timeline: ~1300 cycles per step with every byte cache-hot).  Here the four waves never meet
// (same scheme as vbs_spmm_f32_direct_kernel, k_f32_direct.hip):
//   * the packed A slices (row-major, k contiguous) already ARE the per-lane operand layout of v_mfma_f32_32x32x16: lane (lm, g)
//     needs 8 consecutive k of row lm, one 16-byte load; each wave loads the slice itself (the four waves share it through L1);
//   * B (column-major, k contiguous) is the same layout too, but loading it in MFMA shape -- lane (lm, g) its own column --
//     touches 32 different cache lines per wave instruction, and the texture addresser then sets the pace (round 1's form of
//     this kernel: 36.0 us on the flagship).  So a wave loads ITS 32 columns 4 (KP = 32) or 8 (KP = 64) lanes per column,
//     writes them to a wave-PRIVATE LDS image Bs[column][k] (+8 padding) and reads its fragments back with ds_read_b128:
//     program order and lgkmcnt are all the synchronisation there is.
// Loads run three steps ahead (A: four register sets, B: two staging sets + two LDS stages); step records: one window VGPR,
// constant-lane v_readlane.  Same plans, accumulator layout, epilogue and fix-up as the other stream kernels.
// The body lives in k_h16_direct.inc: this file compiles the plain form, k_h16_live.hip the live form (vbs_fwdlive_h16_kernel).
// =====================================================================================================
#define H16_DIRECT_KERNEL vbs_spmm_h16_direct_kernel
#define H16_DIRECT_LIVE 0
#include "k_h16_direct.inc"
#undef H16_DIRECT_KERNEL
#undef H16_DIRECT_LIVE

// zero-padded copy of the rows of a 16-bit column-major B that face the last (partial) block column: B_tail[k + w j], k < w
__global__ __launch_bounds__(kThreads) void vbs_tail_copy_h16_kernel(const uint16_t* B, int64_t ldb, int64_t row0, int64_t cols, int w, int N,
                                                                     uint16_t* B_tail) {
    const int64_t total = (int64_t)w * N;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t k = e % w, j = e / w;
        B_tail[e] = (row0 + k < cols) ? B[row0 + k + j * ldb] : (uint16_t)0;
    }
}

// the column tail of a 16-bit product whose n_cols is not a multiple of 128: C[:, col0 + j] (+)= Ct[:, j], j < n_t (Ct column-major, ld = rows)
__global__ __launch_bounds__(kThreads) void vbs_col_tail_merge_kernel(const float* Ct, int64_t rows, float* C, int64_t ldc, int c_row_major, int col0,
                                                                      int n_t, int accumulate) {
    const int64_t total = rows * (int64_t)n_t;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        // column-major C: consecutive threads walk a column (coalesced on both sides); row-major C: consecutive threads walk a row of C
        const int64_t r = c_row_major ? e / n_t : e % rows;
        const int j = (int)(c_row_major ? e % n_t : e / rows);
        float* dst = c_row_major ? C + r * ldc + col0 + j : C + r + (int64_t)(col0 + j) * ldc;
        const float v = Ct[r + (int64_t)j * rows];
        *dst = accumulate ? *dst + v : v;
    }
}

// fp32 -> fp16 / bf16 (round to nearest even), column by column: src ld_in, dst ld_out (host-pointer convenience path)
template <bool BF16>
__global__ __launch_bounds__(kThreads) void vbs_convert_h16_kernel(const float* src, int64_t ld_in, int64_t rows, int64_t n_cols, uint16_t* dst,
                                                                   int64_t ld_out) {
    const int64_t total = rows * n_cols;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t k = e % rows, j = e / rows;
        const float v = src[k + j * ld_in];
        uint16_t o;
        if constexpr (BF16) {
            uint32_t u = __float_as_uint(v);
            if ((u & 0x7fffffffu) > 0x7f800000u) o = (uint16_t)((u >> 16) | 0x40);          // NaN stays NaN
            else o = (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
        } else {
            const _Float16 h = (_Float16)v;
            o = __builtin_bit_cast(uint16_t, h);
        }
        dst[k + j * ld_out] = o;
    }
}

template <int KP, bool MI2, bool DEEP>
void launch_h16_d(bool bf16, bool gathered, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (gathered) {
        if (bf16) hipLaunchKernelGGL((vbs_spmm_h16_stream_kernel<KP, MI2, true, true, DEEP>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_spmm_h16_stream_kernel<KP, MI2, false, true, DEEP>), grid, dim3(kThreads), 0, st, sp);
    } else {
        if (bf16) hipLaunchKernelGGL((vbs_spmm_h16_stream_kernel<KP, MI2, true, false, DEEP>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_spmm_h16_stream_kernel<KP, MI2, false, false, DEEP>), grid, dim3(kThreads), 0, st, sp);
    }
}
// SPARTA_H16_DEPTH=4 selects the four-register-set pipeline (loads 5 steps ahead); default: two sets, 3 steps ahead -- measured equal
// within 1 % on every shape (scripts/h16_depth_ab.py): the 16-bit steps are not bound by the bytes in flight
bool h16_deep() { const char* e = std::getenv("SPARTA_H16_DEPTH"); return e && atoi(e) == 4; }   // read per launch: scripts flip it between timings
// Which 16-bit kernel: the no-barrier kernel (vbs_spmm_h16_direct_kernel) for every shape -- flagship 23.0 us against 36.7 for the LDS-staged
// kernel, 64 x 64 blocks 23.7 against 27.8, (w 64, 32 rows) 22.9 against 30.9, N = 256 46 against 53-71; SPARTA_H16_PATH=lds selects the
// LDS-staged kernel (A/B runs, tests).  Read per launch: scripts flip it between timings.
bool h16_direct(int kp, bool mi2) {
    const char* e = std::getenv("SPARTA_H16_PATH");
    if (e && e[0] == 'l') return false;
    return true;
}
// SPARTA_H16_AHEAD=7: the <= 32-row tiles of 32-wide blocks load seven steps ahead instead of three (DEEP).  Measured on the flagship, interleaved
// runs: 22.9 -> 22.1 us while a step still cost 50 instructions, 21.3 -> 21.8 us since it costs 26 (TAIL = false, slices in step order); banded 200k
// through the C ring 30.7 -> 31.4 us.  Off by default; read per launch (scripts flip it between timings).
bool h16_ahead7() { const char* e = std::getenv("SPARTA_H16_AHEAD"); return e && atoi(e) == 7; }
template <int KP, bool MI2, bool GATHERED, bool CSTAGE, bool DEEP, int WC = 32>
void launch_h16_direct_v(bool bf16, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (sp.B_tail != nullptr) {                          // some step reads the zero-padded copy of the last rows of B
        if (bf16) hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<KP, MI2, true, GATHERED, CSTAGE, DEEP, true, WC>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<KP, MI2, false, GATHERED, CSTAGE, DEEP, true, WC>), grid, dim3(kThreads), 0, st, sp);
    } else {
        if (bf16) hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<KP, MI2, true, GATHERED, CSTAGE, DEEP, false, WC>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<KP, MI2, false, GATHERED, CSTAGE, DEEP, false, WC>), grid, dim3(kThreads), 0, st, sp);
    }
}
template <int KP, bool MI2>
void launch_h16_direct(bool bf16, bool gathered, bool c_stage, bool wide, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if constexpr (!MI2 && KP == 32) {
        if (wide) {                                      // the plan holds two sub-worker ranges per workgroup (vbs_plan.cpp, wide16): this kernel and no other
            if (gathered) launch_h16_direct_v<KP, false, true, false, false, 64>(bf16, grid, st, sp);
            else launch_h16_direct_v<KP, false, false, false, false, 64>(bf16, grid, st, sp);
            return;
        }
    }
    if constexpr (!MI2) {
        if (c_stage && !gathered) {                      // tiles of arbitrary height, column-major C: through the C ring (short tiles: seven steps ahead
            launch_h16_direct_v<KP, false, false, true, false>(bf16, grid, st, sp);     // measured slower there, banded 200k 31.4 against 30.7 us)
        } else if (gathered) {
            launch_h16_direct_v<KP, false, true, false, false>(bf16, grid, st, sp);
        } else {
            constexpr bool kCanDeep = KP == 32;          // (64-wide blocks: eight A sets + eight staging sets are 256 registers)
            if (kCanDeep && h16_ahead7()) launch_h16_direct_v<KP, false, false, false, kCanDeep>(bf16, grid, st, sp);
            else launch_h16_direct_v<KP, false, false, false, false>(bf16, grid, st, sp);
        }
    } else {
        if (gathered) launch_h16_direct_v<KP, true, true, false, false>(bf16, grid, st, sp);
        else launch_h16_direct_v<KP, true, false, false, false>(bf16, grid, st, sp);
    }
}
template <int KP, bool MI2>
void launch_h16(bool bf16, bool gathered, bool c_stage, bool wide, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (h16_direct(KP, MI2) || wide) { launch_h16_direct<KP, MI2>(bf16, gathered, c_stage, wide, grid, st, sp); return; }
    if (h16_deep()) launch_h16_d<KP, MI2, true>(bf16, gathered, grid, st, sp);
    else launch_h16_d<KP, MI2, false>(bf16, gathered, grid, st, sp);
}

}  // namespace

namespace sparta_dev {

bool h16_uses_direct_kernel(int kp, bool mi2) { return h16_direct(kp, mi2); }

// Whether the kernel launch_h16_stream picks for (kp, mi2, c_stage, wide) and a B that is not gathered has a live sibling in k_h16_live.hip: the no-barrier
// kernel, three steps ahead.  Not the LDS-staged kernel (SPARTA_H16_PATH=lds) and not DEEP (SPARTA_H16_AHEAD=7, which launch_h16_direct takes for one-tile
// plans of 32-wide blocks outside the ring).
bool h16_live_form_available(int kp, bool mi2, bool c_stage, bool wide) {
    if (!h16_direct(kp, mi2) && !wide) return false;
    if (!mi2 && kp == 32 && !wide && !c_stage && h16_ahead7()) return false;
    return true;
}

void launch_h16_stream(int kp, bool mi2, bool bf16, bool gathered, bool c_stage, bool wide, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (kp == 64) { if (mi2) launch_h16<64, true>(bf16, gathered, false, false, grid, st, sp); else launch_h16<64, false>(bf16, gathered, c_stage, false, grid, st, sp); }
    else { if (mi2) launch_h16<32, true>(bf16, gathered, false, false, grid, st, sp); else launch_h16<32, false>(bf16, gathered, c_stage && !wide, wide, grid, st, sp); }
}

void launch_h16_slab256(bool bf16, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (sp.B_tail != nullptr) {
        if (bf16) hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<32, false, true, false, false, false, true, 64, true>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<32, false, false, false, false, false, true, 64, true>), grid, dim3(kThreads), 0, st, sp);
    } else {
        if (bf16) hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<32, false, true, false, false, false, false, 64, true>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<32, false, false, false, false, false, false, 64, true>), grid, dim3(kThreads), 0, st, sp);
    }
}

// 64-row tiles over 256-column slabs, four accumulators per wave (QUAD): grid = (workers, n_cols / 256).  KP = 64: 64-wide blocks (the hub of a power-law matrix);
// KP = 32: the pair tiles of 32-wide blocks (vbs_plan.cpp)
template <int KP>
static void launch_h16_quad_t(bool bf16, bool gathered, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (gathered) {                                      // (a gathered B has no partial last block column: cols = n_shards * shard_rows, shard_rows % w == 0)
        if (bf16) hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<KP, true, true, true, false, false, false, 64, true>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<KP, true, false, true, false, false, false, 64, true>), grid, dim3(kThreads), 0, st, sp);
    } else if (sp.B_tail != nullptr) {
        if (bf16) hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<KP, true, true, false, false, false, true, 64, true>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<KP, true, false, false, false, false, true, 64, true>), grid, dim3(kThreads), 0, st, sp);
    } else {
        if (bf16) hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<KP, true, true, false, false, false, false, 64, true>), grid, dim3(kThreads), 0, st, sp);
        else hipLaunchKernelGGL((vbs_spmm_h16_direct_kernel<KP, true, false, false, false, false, false, 64, true>), grid, dim3(kThreads), 0, st, sp);
    }
}
void launch_h16_quad(int kp, bool bf16, bool gathered, dim3 grid, hipStream_t st, const StreamParams& sp) {
    if (kp == 64) launch_h16_quad_t<64>(bf16, gathered, grid, st, sp);
    else launch_h16_quad_t<32>(bf16, gathered, grid, st, sp);
}

void launch_tail_copy_h16(hipStream_t st, const uint16_t* B, int64_t ldb, int64_t row0, int64_t cols, int w, int N, uint16_t* B_tail) {
    hipLaunchKernelGGL(vbs_tail_copy_h16_kernel, dim3(32), dim3(kThreads), 0, st, B, ldb, row0, cols, w, N, B_tail);
}

void launch_col_tail_merge(hipStream_t st, const float* Ct, int64_t rows, float* C, int64_t ldc, int c_row_major, int col0, int n_t, int accumulate) {
    const int64_t total = rows * (int64_t)n_t;
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (total + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(vbs_col_tail_merge_kernel, dim3(g), dim3(kThreads), 0, st, Ct, rows, C, ldc, c_row_major, col0, n_t, accumulate);
}

void launch_convert_h16(bool bf16, hipStream_t st, const float* src, int64_t ld_in, int64_t rows, int64_t n_cols, uint16_t* dst, int64_t ld_out) {
    if (bf16) hipLaunchKernelGGL((vbs_convert_h16_kernel<true>), dim3(1024), dim3(kThreads), 0, st, src, ld_in, rows, n_cols, dst, ld_out);
    else hipLaunchKernelGGL((vbs_convert_h16_kernel<false>), dim3(1024), dim3(kThreads), 0, st, src, ld_in, rows, n_cols, dst, ld_out);
}

}  // namespace sparta_dev
