// k_h16_direct.inc -- the body of the no-barrier 16-bit stream kernel, compiled twice: k_h16.hip defines H16_DIRECT_KERNEL = vbs_spmm_h16_direct_kernel and
// H16_DIRECT_LIVE = 0 (the plain form), k_h16_live.hip H16_DIRECT_KERNEL = vbs_fwdlive_h16_kernel and H16_DIRECT_LIVE = 1 (the live form, which walks the
// compacted records of sparta_vbs_set_live_forward).  The live form differs in two places, both behind `if constexpr (LIVE)` or a constant-folded LIVE term,
// so that the plain form compiles to what it compiled to before the body moved here:
//   * a step's slice of A is addressed by its own record (compaction leaves gaps between the slices a worker walks), not by one running offset;
//   * the absent flags mean DEAD: on one-tile records STEP_LO_ABSENT marks the whole step (zero-record descriptors for A and B, B fragments ANDed with 0),
//     on pair tiles a step with both flags set fetches no B either.
// k_h16_a8.hip compiles the body a third time: H16_DIRECT_KERNEL = vbs_fwda8_h16_kernel, H16_DIRECT_A8 = 1 (the a8 form of sparta_vbs_set_forward_a8, DESIGN.md
// section 3.17).  p.A is then the e4m3 image -- the slices in the same order and chunk order, ONE byte per element, so an element offset is a byte offset -- and
// p.steps the handle's private copy of the records, whose last word (the shard index of gathered lists: unread here) holds the biased exponents of the slice's
// two groups, rows 0..31 in bits 0..15 and rows 32..63 in bits 16..31.  The a8 form differs in how a step gets its A fragments and nowhere else: 8-byte loads
// into half as many registers, two scalar shifts for the scales, and four v_cvt_scalef32_pk_{f16,bf16}_fp8 per fragment right in front of its MFMAs.  All of it
// sits behind `if constexpr (A8)` or a constant-folded A8 term.
// k_h16_a8_live.hip compiles it a fourth time: H16_DIRECT_KERNEL = vbs_fwdq8lv_h16_kernel, H16_DIRECT_LIVE = 1 and H16_DIRECT_A8 = 1 (sparta_vbs_set_a8_live,
// DESIGN.md section 3.18).  The two sets of terms compose as they stand: p.steps are the compacted records, a step's offset from its own record is a byte offset
// into the e4m3 image, a dead half reads codes of 0 (+0.0 under any scale) through the zero-record descriptor, and the scales come from the last word of the
// compacted record, where vbs_q8lv_scales_kernel keeps them.
#ifndef H16_DIRECT_A8
#define H16_DIRECT_A8 0
#endif
#ifndef SPARTA_H16_ACCA
#define SPARTA_H16_ACCA 1     // four-accumulator kernels: accumulators pinned to AGPRs (inline-assembly MFMA)
#endif
#ifndef SPARTA_H16_ILV
#define SPARTA_H16_ILV 1      /* two-tile (pair / hub) instantiations: the step's LDS writes and loads between its MFMAs, held there by scheduling barriers */
#endif
#ifndef SPARTA_H16_PROBE
#define SPARTA_H16_PROBE 0        /* developer probes, TIMING ONLY (results wrong): 1 no B loads, 2 no A loads, 4 no epilogue, 8 no LDS round trip, 64 every tile stores to the first rows of C, 128 every step reads the first slice of A, 256 every step reads the first rows of B, 512 one store per tile instead of 16 (non-temporal path) */
#endif

// DEEP: loads 7 steps ahead of their MFMAs instead of 3 (eight A sets, six live B staging sets, two record windows, rounds of eight steps).  A 16-bit
// step of a 32-wide block is two MFMAs (64 cycles) and ~300 cycles of a wave's time: three steps ahead are ~0.4 us, less than a loaded HBM access.
// TAIL = false: no block column hangs over the last row of B (cols % w == 0), the steps never read B_tail -- with the slices of A in step order
// (vbs_plan.cpp) a step then costs 30 scalar / vector instructions around its loads and MFMAs instead of 50, and ONE wave per SIMD issues one
// instruction per ~5 cycles: with neither A nor B loaded the flagship's kernel still took 11.9 of its 22.2 us (SPARTA_H16_PROBE = 3).
// WC = 64 (one-tile plans of 32-wide blocks, vbs_plan.cpp `wide16`): a wave owns 64 columns of the slab, the workgroup's wave pairs (0, 1) and (2, 3) are two
// SUB-WORKERS with their own step ranges -- two tiles per CU at a time, the slice of A through L1 twice instead of four times, and the ~20 instructions a
// step spends on records, addresses and waits pay for four MFMAs instead of two.  Nothing else changes: there is no barrier for the pairs to meet at.
// SLAB (with WC = 64): the four waves work on ONE tile again, 64 columns each -- a 256-column slab per workgroup (grid.y = N / 256), so that A is read once per 256
// columns of B instead of once per 128.  Runs on either plan (the two sub-worker ranges of a workgroup are adjacent); plans without split tiles only.
// SLAB with MI2 (round 3; 64-row tiles, the dense hub of a power-law matrix): FOUR accumulators per wave -- rows 0..31 / 32..63 x the wave's two groups of 32
// columns -- so that a step's slice of A (64 x KP) and its panel of B (KP x 64 per wave) feed 4 NK MFMAs instead of 2 NK: A is read once per 256 columns of B,
// B fragments are used twice.  One workgroup per CU (the 16-bit plans' own choice): the accumulators live in the upper half of the 512-register file.
// Split tiles are allowed: a wave writes its 64 x 64 piece into the slot images of the two 128-column slabs its workgroup covers, in the layout the
// fix-up kernel reads (four waves x 32 columns).
// a chunk of A as the image holds it (16 bytes of 16-bit values / 8 bytes of e4m3 codes) and as the MFMA takes it
template <bool A8>
__device__ __forceinline__ std::conditional_t<A8, u32x2, u32x4> h16_load_chunk(const __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    if constexpr (A8) return __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
    else return __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
}
template <bool BF16>
__device__ __forceinline__ u32x4 h16_widen(const u32x4& c, float) { return c; }
template <bool BF16>
__device__ __forceinline__ u32x4 h16_widen(const u32x2& c, float sc) {        // code x scale, two values per instruction (word_sel: the low / high pair of a dword)
    if constexpr (BF16) return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], sc, false)),
                                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], sc, true)),
                                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], sc, false)),
                                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], sc, true))};
    else return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[0], sc, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[0], sc, true)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[1], sc, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[1], sc, true))};
}

template <int KP, bool MI2, bool BF16, bool GATHERED, bool CSTAGE = false, bool DEEP = false, bool TAIL = true, int WC = 32, bool SLAB = false>
__global__ __launch_bounds__(kThreads, (MI2 && WC == 64) ? 1 : 2) void H16_DIRECT_KERNEL(const StreamParams p) {
    constexpr bool LIVE = H16_DIRECT_LIVE != 0;
    constexpr bool A8 = H16_DIRECT_A8 != 0;
    static_assert(!A8 || (!GATHERED && !DEEP && !(MI2 && WC == 64)), "the a8 forms: B not gathered, three steps ahead, no four-accumulator form");
    constexpr int ACH = A8 ? 8 : 16;                     // bytes of one chunk (8 consecutive k of one row) in the image of A
    static_assert(!SLAB || WC == 64, "256-column slabs are four 64-column waves");
    static_assert(!(CSTAGE && MI2), "the C ring holds 64 rows: tiles of <= 32 rows only");
    static_assert(WC == 32 || (WC == 64 && !CSTAGE && !DEEP && (!MI2 || SLAB)), "64-column waves: without ring, three steps ahead; two-tile form as 256-column slabs only");
    constexpr bool QUAD = MI2 && WC == 64;               // four accumulators per wave
    constexpr int NG = WC / 32;                          // column groups of 32 per wave
    constexpr int D = DEEP ? 7 : 3;                      // steps between a step's loads and its MFMAs
    constexpr int TN = kTN, TM = MI2 ? 64 : 32;
    constexpr int NK = KP / 16;                          // MFMAs (k groups of 16) per step and 32-row tile = 16-byte loads per lane and operand
    constexpr int NA = MI2 ? 2 : 1;
    constexpr int LPC = KP / 8;                          // lanes per column of a coalesced B load (16 bytes = 8 k each): 4 or 8
    constexpr int CPI = 64 / LPC;                        // columns per wave instruction: 16 or 8 (NK instructions cover the wave's 32)
    constexpr int RB = (KP + 8) * 2;                     // bytes per column of the LDS image (8 elements of padding: conflict-free b128)
    constexpr int WSTAGE = 32 * RB;                      // bytes per wave and stage
    __shared__ __attribute__((aligned(16))) char lds[4 * 2 * NG * WSTAGE + (CSTAGE ? 4 * kCRingFloats * 4 : 0)];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int lm = lane & 31, g = lane >> 5;
    const int n0 = blockIdx.y * (SLAB ? 2 * TN : TN);
    // WC = 64: sub-worker (wave >> 1) of this workgroup, wave (wave & 1) of its two; SLAB: the whole workgroup walks both sub-ranges (adjacent) or its one range
    const int worker = (WC == 64 && !SLAB) ? 2 * (int)blockIdx.x + __builtin_amdgcn_readfirstlane(wave >> 1) : (int)blockIdx.x;
    const int wv = (WC == 64 && !SLAB) ? (wave & 1) : wave;
    const int s_begin = (SLAB && p.sub_ranges) ? p.worker_range[4 * worker] : p.worker_range[2 * worker];
    const int n = ((SLAB && p.sub_ranges) ? p.worker_range[4 * worker + 3] : p.worker_range[2 * worker + 1]) - s_begin;
    if (n <= 0) return;
    clock_probe(p.clk, 0);
    // split-tile workspace: one image per 128-column slab; a 256-column workgroup of the four-accumulator form covers slabs 2 y and 2 y + 1 (waves 0, 1 / 2, 3)
    float* ws = p.ws + (int64_t)(QUAD ? 2 * (int)blockIdx.y + __builtin_amdgcn_readfirstlane(wave >> 1) : (int)blockIdx.y) * p.ws_slab_stride;
    const uint16_t* A16 = reinterpret_cast<const uint16_t*>(p.A);
    const uint16_t* B16 = reinterpret_cast<const uint16_t*>(p.B);
    const uint16_t* Bt16 = reinterpret_cast<const uint16_t*>(p.B_tail);

    // step records: one window of 8 (lane = 8 * record + field) per round of four steps, see vbs_spmm_f32_direct_kernel
    const int32_t* srec = reinterpret_cast<const int32_t*>(p.steps + s_begin);
    int vwin = srec[lane];
    int vwin1 = DEEP ? srec[64 + lane] : 0;              // DEEP: the following eight records (positions 8 .. 15)
    int vnext = 0;
#define field(pos, f) ((pos) < 8 ? __builtin_amdgcn_readlane(vwin, 8 * ((pos) & 7) + (f)) : __builtin_amdgcn_readlane(vwin1, 8 * ((pos) & 7) + (f)))
    enum { F_AOFF_LO = 0, F_AOFF_HI = 1, F_BROW = 2, F_H = 3, F_CROW = 4, F_FLAGS = 5, F_SLOT = 6, F_SHARD = 7 };

    const int bc = lane / LPC, bk = (lane % LPC) * 8;    // B load q: column CPI q + bc of the wave's 32, k = bk .. bk + 7
    const int64_t ld_t = (int64_t)p.w;                   // leading dimension of B_tail
    // this wave's 32 columns start at column nw of B / C: folded into the SCALAR bases, so that the 32-bit per-lane offsets only span 32 columns
    // (a column-major B or C with a leading dimension of 2^23 -- configs[4] on one GPU -- is 2 GB per 128 columns, beyond a 32-bit offset)
    const int nw = n0 + WC * __builtin_amdgcn_readfirstlane(wv);
    const uint32_t voffB = (uint32_t)((bc * p.ldb + bk) * 2);
    const uint32_t voffBt = (uint32_t)(((n0 + WC * wv + bc) * ld_t + bk) * 2);
    const uint32_t qstepB = (uint32_t)(CPI * p.ldb * 2), qstepBt = (uint32_t)(CPI * ld_t * 2);      // bytes from one column group to the next
    const uint32_t gstepB = (uint32_t)(32 * p.ldb * 2), gstepBt = (uint32_t)(32 * ld_t * 2);        // ... from one group of 32 columns to the next (WC = 64)
    const uint32_t voffA = (uint32_t)((g * TM + lm) * ACH);     // slice in memory: [k chunk = 2 q + g][row][8]: a wave load is one (TM = 32) or two contiguous pieces
    const int64_t n0off = (int64_t)nw * p.ldb;
    const uint32_t voffC = p.c_row_major ? (uint32_t)((lm * p.ldc + 4 * g) * 4) : (uint32_t)((lm + (4 * g) * p.ldc) * 4);
    char* const ldsw = lds + wave * (2 * NG * WSTAGE);   // this wave's two stages (NG images of 32 columns each)
    const uint32_t lwB = (uint32_t)(bc * RB + bk * 2);   // write: column bc + CPI q
    const uint32_t lrB = (uint32_t)(lm * RB + 16 * g);   // read: column lm, k = 16 q + 8 g .. + 7

    CRing cr;                                            // CSTAGE: finished tiles wait here for whole aligned blocks of 32 rows (vbs_kernel_common.hpp)
    cr.ring = reinterpret_cast<float*>(lds + 4 * 2 * NG * WSTAGE) + wave * kCRingFloats;

    using afrag_t = std::conditional_t<A8, u32x2, u32x4>;  // a chunk as loaded: 8 codes or 8 16-bit values
    struct ASet { afrag_t a[NA][NK]; };
    struct BSet { u32x4 b[NG * NK]; };
    ASet as0, as1, as2, as3;                             // A fragments of the steps i mod 4
    BSet bs0, bs1;                                       // B staging (steps of even / odd index)

    // the slices of A are laid out in step order: one running offset, taken from the first record of the range
    // (live form: every step's offset comes from its own record, see issue_loads)
    auto a_slice = [&](int64_t off) __attribute__((always_inline)) -> void* {
        if constexpr (A8) return const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(p.A) + off);
        else return const_cast<uint16_t*>(A16 + off);
    };
    auto load_a = [&](const __amdgpu_buffer_rsrc_t r, uint32_t chunk) __attribute__((always_inline)) -> afrag_t {
        return h16_load_chunk<A8>(r, voffA, chunk * (uint32_t)ACH);
    };
    int64_t g_aoff = LIVE ? (int64_t)0 : ((int64_t)(uint32_t)field(0, F_AOFF_LO) | ((int64_t)field(0, F_AOFF_HI) << 32)) - (int64_t)TM * KP;
    uint32_t vo_cur = voffB;
    int32_t tail_prev = 0;
    auto issue_loads = [&](auto pos_tag, BSet& rb, ASet& ra) __attribute__((always_inline)) -> int32_t {
        constexpr int s = decltype(pos_tag)::value;      // position of the step's record in the window
        const int32_t flags = field(s, F_FLAGS);
        if constexpr (LIVE) g_aoff = (int64_t)(uint32_t)field(s, F_AOFF_LO) | ((int64_t)field(s, F_AOFF_HI) << 32);
        else g_aoff += (int64_t)TM * KP;
        const int32_t tail = TAIL && (flags & STEP_TAIL) != 0;
        if (tail != tail_prev) {
            vo_cur = tail ? voffBt : voffB;
            asm volatile("" : "+v"(vo_cur));
            tail_prev = tail;
        }
        const int64_t gk0 = (SPARTA_H16_PROBE & 256) ? 0 : field(s, F_BROW);
        const uint16_t* bptr = tail ? Bt16 + gk0 : B16 + (GATHERED ? (int64_t)field(s, F_SHARD) * p.shard_stride : (int64_t)0) + gk0 + n0off;
        // live form: a step that is dead as a whole (the kept step of an all-dead segment) fetches no panel of B either
        const bool dead_all = LIVE && (MI2 ? (flags & (STEP_LO_ABSENT | STEP_HI_ABSENT)) == (STEP_LO_ABSENT | STEP_HI_ABSENT) : (flags & STEP_LO_ABSENT) != 0);
        const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(bptr), 0, dead_all ? 0 : 0x7ffffff0, 0x00020000);
        const uint32_t qs = tail ? qstepBt : qstepB;
        const uint32_t gs = tail ? gstepBt : gstepB;
        if (SPARTA_H16_PROBE & 128) g_aoff = 0;
        if (!(SPARTA_H16_PROBE & 1)) {
#pragma unroll
            for (int c = 0; c < NG; c++)
#pragma unroll
                for (int q = 0; q < NK; q++) rb.b[c * NK + q] = __builtin_amdgcn_raw_buffer_load_b128(rB, vo_cur, gs * c + qs * q, 0);
        }
        // (pair tiles, vbs_plan.cpp: a half of the slice whose block-row has no block in this column is zeros -- a descriptor of zero records returns them without a fetch;
        // the step then clears the B fragments of that half as well, see `half` below)
        const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(a_slice(g_aoff), 0, ((MI2 || LIVE) && (flags & STEP_LO_ABSENT)) ? 0 : 0x7ffffff0, 0x00020000);
        const __amdgpu_buffer_rsrc_t rA1 = __builtin_amdgcn_make_buffer_rsrc(a_slice(g_aoff), 0, (MI2 && (flags & STEP_HI_ABSENT)) ? 0 : 0x7ffffff0, 0x00020000);
        if (!(SPARTA_H16_PROBE & 2) && !((SPARTA_H16_PROBE & 16) && wave != 0) && !((SPARTA_H16_PROBE & 32) && (wave & 1))) {   // 16: only wave 0 loads A; 32: waves 0 and 2
#pragma unroll
            for (int mi = 0; mi < NA; mi++)
#pragma unroll
                for (int q = 0; q < NK; q++) ra.a[mi][q] = load_a(mi == 0 ? rA : rA1, (uint32_t)(2 * q * TM + 32 * mi));
        }
        return flags;
    };
    auto write_b = [&](auto stage_tag, const BSet& rb) __attribute__((always_inline)) {
        constexpr int ST = decltype(stage_tag)::value;
#pragma unroll
        for (int c = 0; c < NG; c++)
#pragma unroll
            for (int q = 0; q < NK; q++) *reinterpret_cast<u32x4*>(ldsw + lwB + (ST * NG + c) * WSTAGE + q * CPI * RB) = rb.b[c * NK + q];
    };

    f32x16 acc0, acc1, acc2, acc3;                        // QUAD: acc0 / acc1 = rows 0..31 / 32..63 of the first 32 columns, acc2 / acc3 of the second
#pragma unroll
    for (int r = 0; r < 16; r++) { acc0[r] = 0.0f; acc1[r] = 0.0f; acc2[r] = 0.0f; acc3[r] = 0.0f; }
    if constexpr (SPARTA_H16_ACCA && QUAD) asm volatile("" : "+a"(acc0), "+a"(acc1), "+a"(acc2), "+a"(acc3));
    // The four-accumulator instantiations run one work-group per CU (up to 512 registers a lane: 256 VGPRs + 256 AGPRs).  Left to itself the register allocator keeps the
    // accumulators in VGPRs between steps and copies all of them into AGPRs and back around every step's MFMAs (16 x NA x NG v_accvgpr_write + as many reads per
    // step).  ACC_A pins them: the MFMA is issued as inline assembly whose accumulator operand is constrained to the AGPRs ("+a"), so the accumulators never leave
    // them until the tile's epilogue.  The hazard recogniser does not look inside inline assembly: the wait states an MFMA result needs before a VALU read
    // (v_accvgpr_read in the epilogue) and a VALU write needs before an MFMA read (the zeroing) are written out as s_nop below.
    constexpr bool ACC_A = SPARTA_H16_ACCA && QUAD;
    auto mfma = [&](const u32x4& bf, const u32x4& af, f32x16& acc) __attribute__((always_inline)) {
        if constexpr (ACC_A) {
            // (s_nop 1: a fragment the allocator parked in AGPRs comes back through v_accvgpr_read right in front of the MFMA: a VALU write needs two wait states
            // before an MFMA reads the register)
            if constexpr (BF16) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(bf), "v"(af));
            else asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(bf), "v"(af));
        } else {
            if constexpr (BF16) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, bf), __builtin_bit_cast(bf16x8, af), acc, 0, 0, 0);
            else acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, bf), __builtin_bit_cast(f16x8, af), acc, 0, 0, 0);
        }
    };

    int32_t fq0 = 0, fq1 = 0, fq2 = 0, fq_new = 0;
    // one step (index i mod 4 = u): fragments of B from LDS stage u & 1, the next step's panel into the other stage, the MFMAs, the
    // tile epilogue if it ends here, then staging set nb and A set na are refilled with step i + D (wb = the set that holds step i + 1: the same as nb for D = 3)
    auto step = [&](auto u_tag, int32_t flags, ASet& wa, BSet& wb, BSet& nb, ASet& na) __attribute__((always_inline)) {
        constexpr int i = decltype(u_tag)::value;
        constexpr int PAR = i & 1;
        u32x4 fb[NG * NK];
        if (SPARTA_H16_PROBE & 8) {
#pragma unroll
            for (int q = 0; q < NG * NK; q++) fb[q] = wb.b[q];
        } else {
#pragma unroll
            for (int c = 0; c < NG; c++)
#pragma unroll
                for (int q = 0; q < NK; q++) fb[c * NK + q] = *reinterpret_cast<const u32x4*>(ldsw + lrB + (PAR * NG + c) * WSTAGE + q * 32);
            if constexpr (!(SPARTA_H16_ILV && MI2 && !DEEP && !TAIL)) write_b(std::integral_constant<int, 1 - PAR>{}, wb);         // W(i + 1)  (two-tile instantiations: between the MFMAs, below)
        }
        constexpr bool ILV = SPARTA_H16_ILV && MI2 && !DEEP && !TAIL && !(SPARTA_H16_PROBE & 8);
        // pair tiles: the half whose block-row has no block in this step's column must not see the panel of B at all.  Its slice of A is zeros, but 0 x Inf and
        // 0 x NaN are NaN: an element of C depends only on the rows of B in block columns that ITS block-row stores (include/sparta_amd.h).  The flags are wave-uniform:
        // the fragments that feed the absent half are ANDed with a scalar 0 (with ~0 otherwise), which clears a NaN as well; no branch around the MFMAs.
        // (live form, one-tile records: STEP_LO_ABSENT marks the whole step dead and every fragment goes through m_lo)
        const uint32_t m_lo = ((MI2 || LIVE) && (flags & STEP_LO_ABSENT)) ? 0u : ~0u, m_hi = (MI2 && (flags & STEP_HI_ABSENT)) ? 0u : ~0u;
        auto half = [&](const u32x4& f, int mi) __attribute__((always_inline)) -> u32x4 {
            if constexpr (!MI2 && !LIVE) return f;
            const uint32_t m = mi == 0 ? m_lo : m_hi;
            return u32x4{f[0] & m, f[1] & m, f[2] & m, f[3] & m};
        };
        // a8 form: the scales of the slice's two groups, 2^e as fp32 bits from the biased exponents in the record (wave-uniform: scalar shifts), and a chunk's 8
        // codes widened to the 16-bit fragment the MFMA takes -- code x scale in one instruction per pair
        float sc_lo = 0.0f, sc_hi = 0.0f;
        if constexpr (A8) {
            const uint32_t ew = (uint32_t)field(i, F_SHARD);
            sc_lo = __uint_as_float((ew & 0xffffu) << 23);
            sc_hi = __uint_as_float((ew >> 16) << 23);
        }
        auto afrag = [&](const afrag_t& c, int mi) __attribute__((always_inline)) -> u32x4 { return h16_widen<BF16>(c, mi == 0 ? sc_lo : sc_hi); };
        if constexpr (!ILV) {
#pragma unroll
            for (int q = 0; q < NK; q++) {
                const u32x4 a_lo = afrag(wa.a[0][q], 0);
                mfma(half(fb[q], 0), a_lo, acc0);
                if constexpr (MI2) mfma(half(fb[q], 1), afrag(wa.a[1][q], 1), acc1);
                if constexpr (WC == 64 && !MI2) mfma(half(fb[NK + q], 0), a_lo, acc1);   // the wave's second 32 columns (acc1: free in the one-tile kernel)
                if constexpr (QUAD) { mfma(half(fb[NK + q], 0), wa.a[0][q], acc2); mfma(half(fb[NK + q], 1), wa.a[1][q], acc3); }
            }
            fq_new = issue_loads(std::integral_constant<int, i + D>{}, nb, na);   // G(i + D)
        } else {
            // ONE wave per SIMD here: nothing but this wave's own instruction order overlaps its MFMAs with the rest of its step.  An MFMA occupies the pipe for 32
            // cycles and takes four to issue: the instruction behind it in program order issues into the other 28.  So: MFMA, one LDS write of the next step's panel
            // (W(i + 1)) or one or two loads of step i + D, MFMA, ... -- kept in that order by scheduling barriers (it is one basic block: the scheduler would
            // cluster the MFMAs again).  TAIL = false instantiations only (no B_tail switch: no branch inside the step).
            constexpr int NM = NK * NA * NG;                 // MFMAs of the step: 4 (pair tiles of 32-wide blocks), 8, 16 (hub tiles)
            constexpr int NW = NG * NK, NLB = NG * NK, NLA = NA * NK;
            const int32_t flags_n = field(i + D, F_FLAGS);
            if constexpr (LIVE) g_aoff = (int64_t)(uint32_t)field(i + D, F_AOFF_LO) | ((int64_t)field(i + D, F_AOFF_HI) << 32);
            else g_aoff += (int64_t)TM * KP;
            if (SPARTA_H16_PROBE & 128) g_aoff = 0;
            const int64_t gk0 = (SPARTA_H16_PROBE & 256) ? 0 : field(i + D, F_BROW);
            const uint16_t* bptr = B16 + (GATHERED ? (int64_t)field(i + D, F_SHARD) * p.shard_stride : (int64_t)0) + gk0 + n0off;
            const bool dead_all_n = LIVE && (flags_n & (STEP_LO_ABSENT | STEP_HI_ABSENT)) == (STEP_LO_ABSENT | STEP_HI_ABSENT);
            const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(bptr), 0, dead_all_n ? 0 : 0x7ffffff0, 0x00020000);
            const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(a_slice(g_aoff), 0, (flags_n & STEP_LO_ABSENT) ? 0 : 0x7ffffff0, 0x00020000);
            const __amdgpu_buffer_rsrc_t rA1 = __builtin_amdgcn_make_buffer_rsrc(a_slice(g_aoff), 0, (flags_n & STEP_HI_ABSENT) ? 0 : 0x7ffffff0, 0x00020000);
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, NM>([&](auto t_tag) __attribute__((always_inline)) {
                constexpr int t = decltype(t_tag)::value;
                constexpr int q = t / (NA * NG), c = (t / NA) % NG, mi = t % NA;       // k group, column group, row half
                f32x16& acc = (c == 0) ? (mi == 0 ? acc0 : acc1) : (mi == 0 ? acc2 : acc3);
                mfma(half(fb[c * NK + q], mi), afrag(wa.a[mi][q], mi), acc);
                __builtin_amdgcn_sched_barrier(0);
                // what goes behind MFMA t: first the NW writes of W(i + 1), then the loads of step i + D spread over the remaining MFMAs
                constexpr int slots = NM;
                constexpr int per_w = (NW + slots / 2 - 1) / (slots / 2);             // writes per slot in the first half
                if constexpr (t < slots / 2) {
#pragma unroll
                    for (int x = t * per_w; x < (t + 1) * per_w && x < NW; x++)
                        *reinterpret_cast<u32x4*>(ldsw + lwB + ((1 - PAR) * NG + x / NK) * WSTAGE + (x % NK) * CPI * RB) = wb.b[x];
                } else {
                    constexpr int h = t - slots / 2, nh = slots - slots / 2;
                    constexpr int lb0 = h * NLB / nh, lb1 = (h + 1) * NLB / nh, la0 = h * NLA / nh, la1 = (h + 1) * NLA / nh;
#pragma unroll
                    for (int x = lb0; x < lb1; x++) nb.b[x] = __builtin_amdgcn_raw_buffer_load_b128(rB, vo_cur, gstepB * (x / NK) + qstepB * (x % NK), 0);
#pragma unroll
                    for (int x = la0; x < la1; x++) na.a[x / NK][x % NK] = load_a((x / NK) == 0 ? rA : rA1, (uint32_t)(2 * (x % NK) * TM + 32 * (x / NK)));
                }
                __builtin_amdgcn_sched_barrier(0);
            });
            fq_new = flags_n;
        }
        if ((flags & STEP_LAST) && !(SPARTA_H16_PROBE & 4)) {
            // the last MFMA's 8 passes + 3 before its accumulator may be read.  The accumulators are operands of the statement: their reads below depend on it
            // (without that the compiler hoists the v_accvgpr_reads common to the branches of the epilogue above it, right behind the last MFMA)
            if constexpr (ACC_A) asm volatile("s_nop 15\n\ts_nop 7" : "+a"(acc0), "+a"(acc1), "+a"(acc2), "+a"(acc3));
            if (flags & STEP_SPLIT) {
                const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(ws + (int64_t)field(i, F_SLOT) * SK_SLOT_FLOATS, 0, SK_SLOT_FLOATS * 4, 0x00020000);
#pragma unroll
                for (int q = 0; q < 16; q++) {
                    if constexpr (QUAD) {               // this wave's 64 columns are the places of waves 2 (wv & 1) and 2 (wv & 1) + 1 in its slab's image (four waves x 32 columns)
                        const uint32_t vt = (uint32_t)((2 * (wv & 1)) * 64 + lane) * 4u;
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc0[q]), rW, vt, (uint32_t)(q * kThreads * 4), 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc2[q]), rW, vt, (uint32_t)(q * kThreads * 4 + 256), 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc1[q]), rW, vt, (uint32_t)((16 + q) * kThreads * 4), 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc3[q]), rW, vt, (uint32_t)((16 + q) * kThreads * 4 + 256), 0);
                    } else if constexpr (WC == 64) {    // the image is laid out for four waves x 32 columns: this wave fills the places of waves 2 wv and 2 wv + 1; rows 32..63: none
                        const uint32_t vt = (uint32_t)((2 * wv) * 64 + lane) * 4u;
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc0[q]), rW, vt, (uint32_t)(q * kThreads * 4), 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc1[q]), rW, vt, (uint32_t)(q * kThreads * 4 + 256), 0);
                        __builtin_amdgcn_raw_buffer_store_b32(0u, rW, vt, (uint32_t)((16 + q) * kThreads * 4), 0);
                        __builtin_amdgcn_raw_buffer_store_b32(0u, rW, vt, (uint32_t)((16 + q) * kThreads * 4 + 256), 0);
                    } else {
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc0[q]), rW, (uint32_t)tid * 4u, (uint32_t)(q * kThreads * 4), 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc1[q]), rW, (uint32_t)tid * 4u, (uint32_t)((16 + q) * kThreads * 4), 0);
                    }
                }
            } else if (CSTAGE) {
                if constexpr (CSTAGE) cr.park(p, nw, lm, g, voffC, acc0, field(i, F_CROW), flags & 0xffff);
            } else {
                const int mt = flags & 0xffff;
                const int64_t c_row = (SPARTA_H16_PROBE & 64) ? 0 : field(i, F_CROW);
                float* cbase = p.c_row_major ? p.C + c_row * p.ldc + nw : p.C + c_row + (int64_t)nw * p.ldc;
                const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc(cbase, 0, 0x7ffffff0, 0x00020000);
                const uint32_t jstep = p.c_row_major ? 4u : (uint32_t)p.ldc * 4u;
                const uint32_t mistep = p.c_row_major ? (uint32_t)p.ldc * 128u : 128u;
#pragma unroll
                for (int cg = 0; cg < NG; cg++) {                              // the wave's groups of 32 columns (WC = 64: two), each with its own scalar base, so that
                    // the per-lane offsets keep spanning 32 columns of C
                    const __amdgpu_buffer_rsrc_t rCm = cg == 1
                        ? __builtin_amdgcn_make_buffer_rsrc(p.c_row_major ? cbase + 32 : cbase + 32 * p.ldc, 0, 0x7ffffff0, 0x00020000) : rC;
#pragma unroll
                    for (int mi = 0; mi < NA; mi++) {                          // rows 0..31 / 32..63 of the tile (MI2)
                        if (mi * 32 + lm < mt) {
                            float v[16];
#pragma unroll
                            for (int q = 0; q < 16; q++) v[q] = QUAD ? (cg == 0 ? (mi == 0 ? acc0[q] : acc1[q]) : (mi == 0 ? acc2[q] : acc3[q]))
                                                                     : ((cg + mi) == 0 ? acc0[q] : acc1[q]);
                            if (p.accumulate) {
                                uint32_t old[16];
#pragma unroll
                                for (int q = 0; q < 16; q++) old[q] = __builtin_amdgcn_raw_buffer_load_b32(rCm, voffC, (uint32_t)((q & 3) + 8 * (q >> 2)) * jstep + (uint32_t)mi * mistep, 0);
#pragma unroll
                                for (int q = 0; q < 16; q++) v[q] += __uint_as_float(old[q]);
                            }
                            if (p.c_nt) {
#pragma unroll
                                for (int q = 0; q < ((SPARTA_H16_PROBE & 512) ? 1 : 16); q++) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q]), rCm, voffC, (uint32_t)((q & 3) + 8 * (q >> 2)) * jstep + (uint32_t)mi * mistep, 2);
                            } else {
#pragma unroll
                                for (int q = 0; q < 16; q++) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[q]), rCm, voffC, (uint32_t)((q & 3) + 8 * (q >> 2)) * jstep + (uint32_t)mi * mistep, 0);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 16; q++) { acc0[q] = 0.0f; acc1[q] = 0.0f; if constexpr (QUAD) { acc2[q] = 0.0f; acc3[q] = 0.0f; } }
            if constexpr (ACC_A) asm volatile("s_nop 4" : "+a"(acc0), "+a"(acc1), "+a"(acc2), "+a"(acc3));
        }
    };

    using c0 = std::integral_constant<int, 0>;
    using c1 = std::integral_constant<int, 1>;
    using c2 = std::integral_constant<int, 2>;
    using c3 = std::integral_constant<int, 3>;
    // the window of steps [i, i + 4): requested one round earlier (4 x NK (NG + NA) loads are issued in between and memory returns in order)
    constexpr int kSwapCnt = 2 * NK * (NG + NA) < 63 ? 2 * NK * (NG + NA) : 63;      // the loads of two steps may stay in flight across the swap
    auto window_swap = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(%1)" : "+v"(vnext) : "n"(kSwapCnt) : "memory");
        vwin = vnext;
    };
    auto window_request = [&](int i) __attribute__((always_inline)) {
        const int32_t* nb = srec + (int64_t)(i + 4) * 8 + lane;
        asm volatile("global_load_dword %0, %1, off" : "=&v"(vnext) : "v"(nb) : "memory");
    };
    if constexpr (DEEP) {
        // step i: LDS stage i & 1, A set i & 7; writes out staging set (i + 1) & 7 and fills staging set and A set (i + 7) & 7 with step i + 7.  Records:
        // window 0 = [8 k, 8 k + 8), window 1 = the next eight (step i + 7 is position 7 of window 0 or 0 .. 6 of window 1); the window after that
        // is requested at the head of a round and swapped in at the head of the next (8 steps' loads are issued in between, memory returns in order:
        // the wait below leaves the loads of seven steps in flight)
        constexpr int kLoadsAhead = D * NK * (1 + NA);
        static_assert(kLoadsAhead <= 63, "vmcnt holds 6 bits");
        ASet asd[8];
        BSet bsd[8];
        int32_t fqd[8];
        auto swap8 = [&]() __attribute__((always_inline)) {
            asm volatile("s_waitcnt vmcnt(%1)" : "+v"(vnext) : "n"(kLoadsAhead) : "memory");
            vwin = vwin1;
            vwin1 = vnext;
        };
        auto request8 = [&](int i) __attribute__((always_inline)) {
            const int32_t* nb = srec + (int64_t)(i + 16) * 8 + lane;
            asm volatile("global_load_dword %0, %1, off" : "=&v"(vnext) : "v"(nb) : "memory");
        };
        static_for<0, 7>([&](auto j) __attribute__((always_inline)) { fqd[j] = issue_loads(j, bsd[j], asd[j]); });
        write_b(c0{}, bsd[0]);                           // W(0)
        const int n8 = n & ~7;
        for (int i = 0; i < n8; i += 8) {
            if (i > 0) swap8();
            request8(i);
            static_for<0, 8>([&](auto u) __attribute__((always_inline)) {
                constexpr int U = decltype(u)::value;
                step(u, fqd[U], asd[U], bsd[(U + 1) & 7], bsd[(U + 7) & 7], asd[(U + 7) & 7]);
                fqd[(U + 7) & 7] = fq_new;
            });
        }
        if (n > n8) {
            if (n8 > 0) swap8();
            const int r = n - n8;
            static_for<0, 7>([&](auto u) __attribute__((always_inline)) {
                constexpr int U = decltype(u)::value;
                if (U < r) {
                    step(u, fqd[U], asd[U], bsd[(U + 1) & 7], bsd[(U + 7) & 7], asd[(U + 7) & 7]);
                    fqd[(U + 7) & 7] = fq_new;
                }
            });
        }
    } else {
        fq0 = issue_loads(c0{}, bs0, as0);
        fq1 = issue_loads(c1{}, bs1, as1);
        write_b(c0{}, bs0);                                  // W(0)
        fq2 = issue_loads(c2{}, bs0, as2);
        const int n4 = n & ~3;
        for (int i = 0; i < n4; i += 4) {
            if (i > 0) window_swap();
            window_request(i);
            step(c0{}, fq0, as0, bs1, bs1, as3);
            fq0 = fq1; fq1 = fq2; fq2 = fq_new;
            step(c1{}, fq0, as1, bs0, bs0, as0);
            fq0 = fq1; fq1 = fq2; fq2 = fq_new;
            step(c2{}, fq0, as2, bs1, bs1, as1);
            fq0 = fq1; fq1 = fq2; fq2 = fq_new;
            step(c3{}, fq0, as3, bs0, bs0, as2);
            fq0 = fq1; fq1 = fq2; fq2 = fq_new;
        }
        if (n > n4) {
            if (n4 > 0) window_swap();
            step(c0{}, fq0, as0, bs1, bs1, as3);
            fq0 = fq1; fq1 = fq2; fq2 = fq_new;
            if (n - n4 >= 2) {
                step(c1{}, fq0, as1, bs0, bs0, as0);
                fq0 = fq1; fq1 = fq2; fq2 = fq_new;
            }
            if (n - n4 == 3) step(c2{}, fq0, as2, bs1, bs1, as1);
        }
    }
    if constexpr (CSTAGE) cr.flush(p, nw, lm, g, voffC, true);
    clock_probe(p.clk, 2);
#undef field
}
