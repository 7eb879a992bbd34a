// vbs_kernel_common.hpp -- device-side helpers shared by the kernel translation units (clock probe, developer timeline
// stamps, accumulator types, step-record field access, the accumulator-image -> C store).
#pragma once
#include "vbs_device.hpp"

namespace sparta_dev {

// ---- k-compaction of the fp32 fragment image: ONE rule for the host packer (vbs_plan.cpp) and the update kernel (k_update.hip) --------------
// `nonempty` bit k: column k of the step's 32-deep slice of A has a non-zero in the tile's rows.  The columns are handed out class by class
// (sequence index s = 4 m + e names column k = 4 m + ((e + m) & 3), so that a class k mod 4 spreads over the four residues of pos mod 4),
// the non-empty ones first; compact index c sits at fragment position (c >> 1) + 16 (c & 1).  The positions are a permutation of 0..31.
__host__ __device__ inline uint32_t frag_seq_mask(uint32_t nonempty) {        // bit s = the sequence's s-th column is non-empty
    uint32_t seq = 0;
    for (int m = 0; m < 8; m++) {
        const uint32_t nib = (nonempty >> (4 * m)) & 15u, r = (uint32_t)(m & 3);
        seq |= (((nib >> r) | (nib << (4 - r))) & 15u) << (4 * m);            // bit e of the group = column bit (e + m) & 3
    }
    return seq;
}
__host__ __device__ inline int frag_position(uint32_t nonempty, int k) {     // fragment position of column k of the slice
    const uint32_t seq = frag_seq_mask(nonempty);
    const int m = k >> 2, s = 4 * m + (((k & 3) - m) & 3);
    const uint32_t before = (1u << s) - 1u;
    const int c = ((nonempty >> k) & 1u) ? __builtin_popcount(seq & before) : __builtin_popcount(seq) + __builtin_popcount(~seq & before);
    return (c >> 1) + 16 * (c & 1);
}
__host__ __device__ inline int frag_pairs(uint32_t nonempty) {               // MFMA pairs the step issues (STEP_KPAIRS holds this - 1)
    const int nk = __builtin_popcount(nonempty), n_mfma = nk + 1 >= 2 ? (nk + 1) / 2 : 1;
    return (n_mfma + 1) / 2;
}

// ---- packed steps of the fp32 one-tile plan (vbs_plan.cpp, k_f32_packed.hip): ONE rule for the planner and the CPU suite -------------------
// A block of a tile is cut into its eight aligned 4-column groups (k = 4 m .. 4 m + 3: the 16-byte pieces a lane loads from column-major B);
// bit m of its mask: the group has a non-zero in the tile's rows.  Whole blocks are packed into steps of at most 8 slots (a slot = one group
// = one MFMA pair), first-fit decreasing by group count, ties in ascending block order; a block without any group takes no slot and rides
// in the first step.  step_of_block / slot0_of_block: the block's step and the slot of its first non-empty group (the others follow in
// ascending m).  Returns the number of steps.  Deterministic, and a function of the masks alone.
inline int32_t f32_pack_blocks(int32_t n_blocks, const uint8_t* masks, int32_t* step_of_block, int32_t* slot0_of_block) {
    int32_t fill[8 + 1];                                  // per group count c = 8 .. 0: the blocks in ascending order come from a counting sort
    std::vector<int32_t> order((size_t)std::max(n_blocks, 0)), used;
    for (int c = 0; c <= 8; c++) fill[c] = 0;
    for (int32_t b = 0; b < n_blocks; b++) fill[__builtin_popcount(masks[b])]++;
    int32_t at = 0, start[9];
    for (int c = 8; c >= 0; c--) { start[c] = at; at += fill[c]; }
    for (int32_t b = 0; b < n_blocks; b++) order[(size_t)start[__builtin_popcount(masks[b])]++] = b;
    for (int32_t q = 0; q < n_blocks; q++) {
        const int32_t b = order[(size_t)q], c = __builtin_popcount(masks[b]);
        size_t s = 0;
        while (s < used.size() && used[s] + c > 8) s++;
        if (s == used.size()) used.push_back(0);
        step_of_block[b] = (int32_t)s;
        slot0_of_block[b] = used[s];
        used[s] += c;
    }
    return (int32_t)used.size();
}

// ---- the fp8 (e4m3) weight image of 16-bit handles (sparta_vbs_set_forward_a8): ONE rule for vbs_a8quant_kernel (k_h16_a8.hip) and the host -----------
// (include/sparta_amd.h states it; integer code throughout, so that ties, subnormals and -0 are the same bits on either side)
// a8_amax_bits: the running maximum of |v| over the FINITE elements of a group, as the bits of a non-negative float (ordered as unsigned integers).
__host__ __device__ inline uint32_t a8_amax_bits(uint32_t amax, uint32_t v_bits) {
    const uint32_t a = v_bits & 0x7fffffffu;
    return (a < 0x7f800000u && a > amax) ? a : amax;
}
// the group's exponent e from its amax: the smallest e with amax * 2^-e <= 448, clamped to [-126, 127]; 0 for amax == 0.  amax = m * 2^x with m in [0.5, 1):
// x = E - 126 for a normal float (m <= 0.875: mantissa field <= 0x600000); a subnormal amax has x <= -126 and clamps to -126.  (No finite fp32 reaches the
// upper clamp: FLT_MAX gives 120.)
__host__ __device__ inline int32_t a8_exponent(uint32_t amax) {
    if (amax == 0u) return 0;
    const int32_t E = (int32_t)(amax >> 23);
    if (E == 0) return -126;
    const int32_t e = E - 126 - ((amax & 0x7fffffu) <= 0x600000u ? 9 : 8);
    return e < -126 ? -126 : (e > 127 ? 127 : e);
}
// 2^-e as fp32 bits (e in [-126, 126]: every e a8_exponent returns)
__host__ __device__ inline uint32_t a8_inv_scale_bits(int32_t e) { return (uint32_t)(127 - e) << 23; }
// the OCP e4m3fn code of x = v * 2^-e (its fp32 bits), round to nearest even: subnormals and the sign of zero kept, NaN and +-Inf the NaN code with their sign;
// |x| <= 448 by the choice of e (anything above would saturate to 448: never taken)
__host__ __device__ inline uint32_t a8_code(uint32_t x_bits) {
    const uint32_t sign = (x_bits >> 24) & 0x80u, a = x_bits & 0x7fffffffu;
    if (a >= 0x7f800000u) return sign | 0x7fu;
    if (a >= (121u << 23)) {                               // |x| >= 2^-6: normal in e4m3 -- 20 mantissa bits go
        const uint32_t r = (a + 0x7ffffu + ((a >> 20) & 1u)) >> 20;
        const uint32_t c = r - (120u << 3);
        return sign | (c > 0x7eu ? 0x7eu : c);
    }
    // |x| < 2^-6: multiples of 2^-9 -- |x| * 512 lies in [0, 8), adding 2^23 rounds it to an integer (to nearest even) in the low mantissa bits
    union { uint32_t u; float f; } t;
    t.u = a;
    t.f = t.f * 512.0f + 8388608.0f;
    return sign | (t.u & 0xfu);
}

}  // namespace sparta_dev

#ifdef __HIP__            // what follows is device code: the host translation units stop here
namespace sparta_dev {

// Clock probe: s_memtime counts shader-clock cycles, s_memrealtime a constant 100 MHz; the ratio over a kernel's lifetime is
// the clock the MFMA pipes actually ran at (the board drops it under a dense fp32 MFMA load: DESIGN.md, "clock").
// Developer instrumentation (make TIMELINE=1 -> libsparta_amd_tl.so; never in the product build): s_memtime stamps inside the steps
// of one workgroup of the fp32 stream kernel, written behind the 16 clock-probe words.  scripts/timeline.py reads them.
#ifdef SPARTA_TIMELINE
#define TL_STEPS 64
#define TL_FIRST 16
#define TL_STAMP(k) do { if (tl_on) asm volatile("s_memtime %0" : "=s"(tl[k])); } while (0)
#else
#define TL_STAMP(k) do { } while (0)
#endif

// Cache policy of the stream kernels' C stores, chosen per launch (StreamParams::c_nt, a scalar branch around the 16 store
// instructions -- stores define no register, so the join costs nothing): NON-TEMPORAL where tiles are long (>= 6 steps per tile on average) --
// C is written once and never read back, with the default policy the 32 MB of C of the flagship push panels of B out of the L2s (fp32
// flagship, same box, interleaved runs: 54.2 -> 53.2 us) -- and the DEFAULT policy where tiles are short: a step's loads wait (vmcnt is one
// in-order counter on gfx9) for the stores of the tile that ended two steps earlier, and non-temporal stores take longer to complete
// (banded 200k, 1.8 steps per tile: 78-79 us non-temporal, 56-68 default; with every tile storing to the same rows of C: 37).

// f(integral_constant<0>) ... f(integral_constant<N - 1>): a loop whose index is a compile-time constant in every iteration
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); static_for<I + 1, N>(f); }
}

__device__ __forceinline__ void clock_probe(long long* clk, int slot) {
    if (clk != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        clk[slot] = (long long)__builtin_readcyclecounter();
        clk[slot + 1] = (long long)wall_clock64();
    }
}

// fp32 -> fp16 / bf16 bits exactly as to_h16 (vbs_plan.cpp) rounds at creation: round to nearest even; bf16 keeps a NaN a NaN (quiet bit set), Inf stays Inf
// (k_update.hip: the 16-bit images; k_epilogue.hip: 16-bit outputs)
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

template <int MF>
struct Acc;
template <>
struct Acc<32> { typedef f32x16 type; };
template <>
struct Acc<16> { typedef f32x4 type; };

__device__ __forceinline__ int32_t sk_field(int vrec0, int vrec1, int s, int f) {   // field f of step s's record (see the kernels)
    const int ln = ((s & 7) << 3) + f;
    const int32_t x0 = __builtin_amdgcn_readlane(vrec0, ln), x1 = __builtin_amdgcn_readlane(vrec1, ln);
    return ((s >> 3) & 1) ? x1 : x0;
}

// D[j][i] register image -> C.  lane: i = lane & 31 (row), g = lane >> 5; register r: j = (r&3) + 8(r>>2) + 4g.
__device__ __forceinline__ void sk_store_tile(const f32x16& acc0, const f32x16& acc1, int mt, int c_row, int col0, float* C,
                                              int64_t ldc, int c_row_major, int accumulate, int lm, int g) {
#pragma unroll
    for (int mi = 0; mi < 2; mi++) {
        const int row = mi * 32 + lm;
        if (row >= mt) continue;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int col = col0 + (r & 3) + 8 * (r >> 2) + 4 * g;
            float* dst = c_row_major ? C + (int64_t)(c_row + row) * ldc + col : C + (int64_t)(c_row + row) + (int64_t)col * ldc;
            float v = mi == 0 ? acc0[r] : acc1[r];
            if (accumulate) v += *dst;
            *dst = v;
        }
    }
}

// ---- the C ring of the no-barrier kernels (CSTAGE: column-major C, tiles of <= 32 rows of arbitrary height) -------------------------------
// A wave does not store a finished tile straight away but parks it in a wave-private ring of 64 rows x its 32 columns in LDS (row of the ring
// = row of C & 63) and stores ALIGNED blocks of 32 rows once the tiles that follow -- a worker walks vertically adjacent tiles -- have
// completed them: whole 128-byte pieces of a column instead of the 28-row pieces of two neighbouring tiles, which the memory side has to
// read, merge and write back and acknowledges late (gfx9 has one in-order counter for loads and stores: the loads of step i + 4 wait for the
// stores of the tile that ended at step i; banded 200k).  The flush is lazy -- at the next tile's epilogue, one site in a
// scalar loop; the block a worker's range starts or ends in, and blocks around a gap between tiles (an empty block-row, sparse rows, a split
// tile), are stored partially, as before.  All state is wave-uniform (scalar registers).
constexpr int kCRingStride = 65;                                 // floats per column of the ring (64 rows + 1)
constexpr int kCRingFloats = 32 * kCRingStride;                  // per wave
struct CRing {
    float* ring;                                                 // element (column j, row r) at j * kCRingStride + (r & 63)
    int32_t win_base = 0, pend_lo = 0, pend_hi = 0;              // rows [pend_lo, pend_hi) of C are parked; win_base = first aligned block not yet stored

    // stores rows [max(b, lo), min(b + 32, hi)) of the aligned block b (lane lm = row b + lm), the way the direct epilogue stores a tile
    __device__ __forceinline__ void flush_block(const StreamParams& p, int n0, int lm, int g, uint32_t voffC, int32_t b, int32_t lo, int32_t hi) {
        float* cbase = p.C + (int64_t)b + (int64_t)n0 * p.ldc;
        const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc(cbase, 0, 0x7ffffff0, 0x00020000);
        const uint32_t jstep = (uint32_t)p.ldc * 4u;
        const int32_t row = b + lm;
        if (row >= lo && row < hi) {
            float v[16];
#pragma unroll
            for (int q = 0; q < 16; q++) v[q] = ring[((q & 3) + 8 * (q >> 2) + 4 * g) * kCRingStride + (row & 63)];
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
    // stores what can be stored: everything parked (`all`: the next tile is not adjacent, or the range ends), else the blocks that are complete
    __device__ __forceinline__ void flush(const StreamParams& p, int n0, int lm, int g, uint32_t voffC, bool all) {
        while (pend_lo < pend_hi && (all || pend_hi - win_base >= 32)) {
            flush_block(p, n0, lm, g, voffC, win_base, pend_lo, pend_hi);
            win_base += 32;
            pend_lo = win_base < pend_hi ? win_base : pend_hi;
        }
    }
    // a finished tile (rows [c_row, c_row + mt) of C, mt <= 32, accumulator image `acc` of this wave's 32 columns) goes into the ring
    __device__ __forceinline__ void park(const StreamParams& p, int n0, int lm, int g, uint32_t voffC, const f32x16& acc, int32_t c_row, int32_t mt) {
        flush(p, n0, lm, g, voffC, pend_lo < pend_hi && c_row != pend_hi);          // (a gap: drain first, the ring restarts at this tile)
        if (pend_lo >= pend_hi) { win_base = c_row & ~31; pend_lo = c_row; }
        if (lm < mt) {
#pragma unroll
            for (int q = 0; q < 16; q++) ring[((q & 3) + 8 * (q >> 2) + 4 * g) * kCRingStride + ((c_row + lm) & 63)] = acc[q];
        }
        pend_hi = c_row + mt;
    }
};

}  // namespace sparta_dev
#endif  // __HIP__
