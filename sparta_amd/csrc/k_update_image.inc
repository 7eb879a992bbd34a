// k_update_image.inc -- the two image kernels of k_update.hip, included once per VALUE SOURCE (the file defines UPD_SOURCE before each inclusion):
//   UPD_SOURCE 0   vbs_update_f32_frag_kernel / vbs_update_h16_kernel: a value is the plain load mab[i] (sparta_vbs_set_values)
//   UPD_SOURCE 1   vbs_sgd_f32_frag_kernel / vbs_sgd_h16_kernel: the values of a lane come from SgdStep::step -- W, G (and M) loaded, the arithmetic done in
//                  registers, W (and M) stored, the new weights returned (sparta_vbs_sgd_step, where the kernel's image holds every stored element exactly once)
//   UPD_SOURCE 2   vbs_adam_f32_frag_kernel / vbs_adam_h16_kernel: the same with AdamStep::step -- W, G, M, V loaded, W, M, V stored (sparta_vbs_adam_step)
// Everything behind the loads -- ballot, k-compaction, rounding, placement -- is the same text.
// UPD_LIVE (defined to 1 around an inclusion with UPD_SOURCE 1 or 2): the live form of the two stepping kernels, vbs_sgdlive_* / vbs_adamlive_*.  One more
// argument, live_words (k_live.hip writes it from the snapshot of the live set): one 32-bit word per step (fp32) / two per slice, its rows 0..31 and its rows
// 32..63 (16-bit: the two block-rows of a pair tile; twice the same block for an ordinary 64-row tile); bit k & 31 says "column k of the step / of those rows
// of the slice lies in a live block".  Wherever an image kernel exists the block width is a multiple of 32: a step is 32 columns of ONE block and a 16-byte chunk 8 columns of one block, so the 16 (8) elements of a lane share one bit (the host refuses to build
// the words otherwise) and the lane tests the bit of its first column: dead, it does not call the value source at all -- nothing loaded, nothing stored, its
// values stay the +0.0f they were initialised to -- and the ballot, the k-compaction and the rounding see zero columns.  Live, it runs the unchanged
// loads-first / arithmetic / stores text of step<N>.  (A test per element inside step<16> was tried first: 328 registers against 248 in the Adam kernel.)
#ifndef UPD_LIVE
#define UPD_LIVE 0
#endif
#if UPD_SOURCE == 1 && !UPD_LIVE
#define UPD_STEP SgdStep
#define UPD_FRAG_KERNEL vbs_sgd_f32_frag_kernel
#define UPD_H16_KERNEL vbs_sgd_h16_kernel
#elif UPD_SOURCE == 2 && !UPD_LIVE
#define UPD_STEP AdamStep
#define UPD_FRAG_KERNEL vbs_adam_f32_frag_kernel
#define UPD_H16_KERNEL vbs_adam_h16_kernel
#elif UPD_SOURCE == 1
#define UPD_STEP SgdStep
#define UPD_FRAG_KERNEL vbs_sgdlive_f32_frag_kernel
#define UPD_H16_KERNEL vbs_sgdlive_h16_kernel
#elif UPD_SOURCE == 2
#define UPD_STEP AdamStep
#define UPD_FRAG_KERNEL vbs_adamlive_f32_frag_kernel
#define UPD_H16_KERNEL vbs_adamlive_h16_kernel
#endif
#if UPD_LIVE
#define UPD_LIVE_ARG , const uint32_t* __restrict__ live_words
#else
#define UPD_LIVE_ARG
#endif

// The forward of vbs_f32_legacy_from_frag_kernel.  One wave per step q of the one-tile plan (four steps per workgroup and pass): lane = (row m = lane & 31,
// half g = lane >> 5).  Load i (0..15) of a lane reads element (m, k = 2 i + g) of the step's slice -- the 32 lanes of a half read 32 consecutive floats of
// one column -- and its ballot gives the "column has a non-zero in the tile's rows" bits of the columns 2 i and 2 i + 1; rows >= mt belong to the next tile of
// the block-row (or to nobody) and are neither read nor counted.  The position table follows from the 32 bits by the rule the host packer uses
// (frag_position).  A stepping source: the values are the NEW weights (rows m < mt of the steps are every stored element once), so the ballot sees it.
// The values go through a 4 KB image in LDS, [position][row], and leave it as the slice wants them: 16-byte quads [row][e = 0..3] of one
// (j, g), 1 KB of consecutive addresses per store instruction.  Empty columns and rows >= mt are stored as zeros (their loads were masked to zero).
#if UPD_SOURCE == 0
__global__ __launch_bounds__(kThreads) void vbs_update_f32_frag_kernel(StepRec* steps, int64_t n_steps, const float* __restrict__ mab, float* __restrict__ a_frag,
                                                                       float* __restrict__ A_out) {
#else
__global__ __launch_bounds__(kThreads) void UPD_FRAG_KERNEL(StepRec* steps, int64_t n_steps, UPD_STEP vs, float* __restrict__ a_frag, float* __restrict__ A_out UPD_LIVE_ARG) {
#endif
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
#if UPD_SOURCE == 0
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int k = 2 * i + g;
            v[i] = m < mt ? mab[a_off + (int64_t)k * h + m] : 0.0f;
            const unsigned long long b = __ballot(v[i] != 0.0f);
            nonempty |= ((uint32_t)b != 0u ? 1u : 0u) << (2 * i) | ((uint32_t)(b >> 32) != 0u ? 1u : 0u) << (2 * i + 1);
        }
#else
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = 0.0f;
#if UPD_LIVE
        if (m < mt && ((live_words[q] >> g) & 1u) != 0u) vs.step<16>(a_off + (int64_t)g * h + m, 2 * h, v);     // (m < mt implies active; bit g: the lane's first column)
#else
        if (m < mt) vs.step<16>(a_off + (int64_t)g * h + m, 2 * h, v);         // element (m, k = 2 i + g), i = 0..15
#endif
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const unsigned long long b = __ballot(v[i] != 0.0f);
            nonempty |= ((uint32_t)b != 0u ? 1u : 0u) << (2 * i) | ((uint32_t)(b >> 32) != 0u ? 1u : 0u) << (2 * i + 1);
        }
#endif
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

// One lane = one 16-byte chunk of one slice: 8 consecutive k of one row.  Chunk c of a slice is (k chunk kc = c / TMS, row rr = c % TMS): neighbouring lanes
// hold neighbouring rows, so each of the 8 loads of a wave reads runs of consecutive floats of one column.  Stream slices store chunk c at c (the layout
// [k / 8][row][8]: consecutive lanes, consecutive chunks); hub slices at the swizzled place of k_hub16.hip's LDS image.  Rows the map does not cover are zeros.
// A stepping source (stream slices only): a lane owns the 8 elements of its chunk, and the chunks of the map's covered rows are every stored element once.
#if UPD_SOURCE == 0
template <bool BF16, bool HUB, int TMS, int KP>
__global__ __launch_bounds__(kThreads) void vbs_update_h16_kernel(const UpdSlice* __restrict__ map, int64_t n_slices, const float* __restrict__ mab, uint16_t* __restrict__ dst) {
#else
template <bool BF16, int TMS, int KP>
__global__ __launch_bounds__(kThreads) void UPD_H16_KERNEL(const UpdSlice* __restrict__ map, int64_t n_slices, UPD_STEP vs, uint16_t* __restrict__ dst UPD_LIVE_ARG) {
    constexpr bool HUB = false;
#endif
    constexpr int kChunks = TMS * KP / 8;
    const int64_t total = n_slices * kChunks, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x; id < total; id += stride) {
        const int64_t s = id / kChunks;
        const int c = (int)(id % kChunks), kc = c / TMS, rr = c % TMS;
#if UPD_LIVE
        // a chunk of a dead block is zeros, as a row the map does not cover: stored at once, in front of everything the live path holds in registers (rr >> 5: rows
        // 0..31 or 32..63 of the slice; stepping sources have no hub form, so the chunk's place is c * 8)
        uint32_t lw;
        if constexpr (kChunks % kThreads == 0) {                // 64-row slices: the kThreads chunks of a workgroup's pass lie in ONE slice, s is uniform and its
            const uint32_t su = __builtin_amdgcn_readfirstlane((uint32_t)(2 * s));      // two words come through the scalar cache (a plan has fewer than 2^31 slices)
            const uint32_t w0 = live_words[su], w1 = live_words[su + 1u];
            lw = rr >= 32 ? w1 : w0;
        } else lw = live_words[(uint32_t)(2 * s) + (uint32_t)(rr >> 5)];
        if (((lw >> ((kc * 8) & 31)) & 1u) == 0u) {
            *reinterpret_cast<u32x4*>(dst + s * (int64_t)(TMS * KP) + c * 8) = u32x4{0u, 0u, 0u, 0u};
            continue;
        }
#endif
        const UpdSlice u = map[s];
#if UPD_SOURCE == 0
        const float* src = nullptr;
        int64_t ld = 0;
        if (rr < u.rows_lo) { src = mab + u.off_lo + rr; ld = u.h_lo; }
        else if (rr >= 32 && rr - 32 < u.rows_hi) { src = mab + u.off_hi + (rr - 32); ld = u.h_hi; }
        u32x4 o = {0u, 0u, 0u, 0u};
        if (src != nullptr) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; e++) x[e] = src[(int64_t)(kc * 8 + e) * ld];
#else
        int64_t at0 = -1, ld = 0;                               // the lane's row: the index of its first element in W, G, M (-1: a row the map does not cover)
        if (rr < u.rows_lo) { at0 = u.off_lo + rr; ld = u.h_lo; }
        else if (rr >= 32 && rr - 32 < u.rows_hi) { at0 = u.off_hi + (rr - 32); ld = u.h_hi; }
        u32x4 o = {0u, 0u, 0u, 0u};
        if (at0 >= 0) {
            float x[8];
            vs.step<8>(at0 + (int64_t)(kc * 8) * ld, ld, x);
#endif
#pragma unroll
            for (int e = 0; e < 4; e++) o[e] = upd_h16<BF16>(x[2 * e]) | (upd_h16<BF16>(x[2 * e + 1]) << 16);
        }
        const int at = HUB ? rr * 64 + ((kc ^ ((rr >> 1) & 7)) << 3) : c * 8;
        *reinterpret_cast<u32x4*>(dst + s * (int64_t)(TMS * KP) + at) = o;
    }
}

#if UPD_SOURCE != 0
#undef UPD_STEP
#undef UPD_FRAG_KERNEL
#undef UPD_H16_KERNEL
#endif
#undef UPD_LIVE_ARG
#undef UPD_LIVE
