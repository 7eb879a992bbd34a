// k_sddmm.hip -- sampled dense-dense product on the stored blocks of a VBS handle (sparta_vbs_sddmm):
//   G[a_off + q * h + i] (+)= sum_n X[c_row + i, n] * Y[jab[b] * w + c, n]      stored column q = b * w + c of the block-row
// the gradient of A's values for C = A * B (X = dC, Y = B).  Same work as the forward product: dense MFMA tiles, the reduction over k.
//
// One workgroup (4 waves) per work item = (block-row, tile of <= 32 of its rows, up to kSdGroups groups of 32 stored columns); wave v takes
// the item's groups v, v + 4, v + 8, v + 12.  Stored columns are taken in mab order, so narrow blocks (w < 32) pack into one group; each lane
// gathers the column of Y its stored column belongs to.  k is walked in chunks of KC: the X tile of the chunk (32 rows x KC) is staged in LDS
// once and read by all four waves for every one of their groups.
//
// The operands are swapped (A operand = Y, B operand = X), so an accumulator holds ROW i = lane & 31 of the tile and stored column
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5) in register r: a store instruction writes 32 consecutive rows of one stored column = 32 consecutive
// floats of mab (no transpose, any alignment).
//
// fp32: v_mfma_f32_32x32x2_f32.  Lane l holds entity l & 31 (row of X / stored column) at k = l >> 5: for a fixed n, 32 consecutive rows of the
//       column-major X (Y) are one coalesced load; Y goes straight to registers, X through the LDS tile [KC][32].
// 16-bit: v_mfma_f32_32x32x16_{f16,bf16} wants 8 consecutive k per lane, which column-major X and Y have strided.  Both are staged as
//       [k][32 entities] images (coalesced row loads; X once per workgroup, Y per wave and group) and read back with ds_read_b64_tr_b16.
//       EXEC is all ones at every transposed read (the group loops are wave-uniform), the LDS image is one 16-byte aligned static object.
//
// Live-block set (sparta_vbs_set_live_blocks, k_live.hip): the LIVE forms of the two kernels (vbs_sdlive_*_kernel; the bodies are templates, LIVE = false
// is the kernel as it always was).  An item takes positions g0 .. g0 + 15 of its block-row's COMPACTED list of live groups; a workgroup whose item has none
// returns before its first barrier; inside a live group a lane whose stored column belongs to a dead block loads nothing and its column is stored as +0.0f
// (accumulate = 0) or skipped, neither read nor written (accumulate = 1).  The groups without a live block are not visited: their zeros under accumulate = 0
// come from a launch of the mask kernel of k_prune.hip on G and the snapshot, in front (vbs_capi.cpp).  (Storing them inside this kernel was built and
// measured: 2 to 6 us faster at the median, inside the arms' ranges -- profiles/live/README.md -- and not kept.)
//
// Score form (sparta_vbs_sddmm_block_ssq; vbs_sdscore_*_kernel): a third mode of the two bodies, the LIVE form on the lists of the call's selection up to the
// end of a group, where the accumulator is not stored but reduced -- sd_score -- to one fp64 sum of squares per stored column, written to a slot of the handle's
// scratch (one per 32-row tile and stored column); vbs_sdscore_finish_kernel, one wave per block, sums a block's slots in one fixed order.  G is not touched.
#include "vbs_kernel_common.hpp"

namespace sparta_dev {

namespace {

constexpr int kSdWaves = 4;
constexpr int kSdGpw = kSdGroups / kSdWaves;      // groups per wave
constexpr int kKC32 = 32;                          // k chunk, fp32 (16 MFMA steps of depth 2)
constexpr int kKC16 = 32;                          // k chunk, 16-bit (2 MFMA steps of depth 16)
constexpr int kSdPlain = 0, kSdLive = 1, kSdScore = 2;   // the modes of the two bodies; kSdScore is kSdLive up to the store

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// the stored column of lane (lane & 31) in group gi of the item: its column of Y, or -1 (past the block-row's stored columns, or ragged); LIVE: -2 if
// its block is dead (keep = the snapshot, one byte per block).  The LIVE form is branch-free -- a lane past the block-row's stored columns looks up block 0,
// which exists: a workgroup gets here only with a group to compute -- so that the loads of the wave's groups (jab and keep of each) are issued together: written
// with the early return of the plain form, every load waits for the one before it, and the eight extra round trips cost the kernel 15 us of its 140
// (profiles/live/README.md)
// ... for NQ stored columns at once, in three phases -- the divisions (a 64-bit division is a routine with a branch of its own), then every load, then the
// classification: the loads of all NQ are in flight together
template <int NQ>
__device__ __forceinline__ void sd_columns_live(const SddmmParams& p, const BlockRowDesc& br, int64_t nq, const int64_t (&q)[NQ], const uint8_t* keep, int64_t (&col)[NQ]) {
    int64_t b[NQ], c[NQ];
    int32_t jb[NQ];
    uint8_t k[NQ];
#pragma unroll
    for (int t = 0; t < NQ; t++) {
        const int64_t qc = q[t] < nq ? q[t] : 0;
        b[t] = qc / p.w;
        c[t] = qc - b[t] * p.w;
    }
#pragma unroll
    for (int t = 0; t < NQ; t++) {
        jb[t] = p.jab[br.jab_off + b[t]];
        k[t] = keep[br.jab_off + b[t]];
    }
#pragma unroll
    for (int t = 0; t < NQ; t++) {
        const int64_t cc = (int64_t)jb[t] * p.w + c[t];
        col[t] = q[t] >= nq ? -1 : k[t] == 0 ? -2 : cc < p.cols ? cc : -1;
    }
}

template <bool LIVE>
__device__ __forceinline__ int64_t sd_column(const SddmmParams& p, const BlockRowDesc& br, int64_t nq, int64_t q, const uint8_t* keep) {
    if constexpr (LIVE) {
        const int64_t qs[1] = {q};
        int64_t col[1];
        sd_columns_live<1>(p, br, nq, qs, keep, col);
        return col[0];
    } else {
        if (q >= nq) return -1;
        const int64_t b = q / p.w, c = q - b * p.w;
        const int64_t col = (int64_t)p.jab[br.jab_off + b] * p.w + c;
        return col < p.cols ? col : -1;
    }
}

// the 32 x 32 accumulator -> G: lane (i = lane & 31, g = lane >> 5), register r: stored column q0 + (r & 3) + 8 (r >> 2) + 4 g, row i.  A stored position past
// cols (ragged last block column) gets 0 whatever X holds: its accumulator is X times the zeros that stand in for a row of Y that does not exist, and
// Inf x 0 is NaN (include/sparta_amd.h: such a position depends on nothing).  LIVE: a second mask, the positions of dead blocks -- +0.0f under
// accumulate = 0, neither read nor written under accumulate = 1; a ragged position of a live block still gets its 0
template <bool LIVE>
__device__ __forceinline__ void sd_store(const SddmmParams& p, const BlockRowDesc& br, const f32x16& acc, float* G, int64_t base, int64_t q0, int64_t nq, int h, int mt,
                                         int lane, int accumulate, const uint8_t* keep) {
    const int i = lane & 31;
    // bit j: stored position q0 + j is a column of the matrix -- looked up once per group of 32 positions (lane j), not once per stored element
    const int64_t cq = sd_column<LIVE>(p, br, nq, q0 + i, keep);
    const unsigned long long live = __ballot(cq >= 0);
    const unsigned long long dead = LIVE ? __ballot(cq == -2) : 0ull;
    if (i >= mt) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int j = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int64_t q = q0 + j;
        if (q >= nq) continue;
        float* dst = G + base + q * h + i;
        if constexpr (LIVE)
            if ((dead >> j) & 1) {
                if (!accumulate) *dst = 0.0f;
                continue;
            }
        const float v = (live >> j) & 1 ? acc[r] : 0.0f;
        *dst = accumulate ? *dst + v : v;
    }
}

// the score form's end of a group: instead of storing, the 32 x 32 accumulator is reduced to one fp64 sum of squares per stored column.  A lane squares its
// sixteen values in fp64 (exact: 24 x 24 bits) under the masks of sd_store -- the column is inside the matrix and of a selected block, the row is one of the
// tile's mt -- and the 32 lanes of a half-wave (the rows of the half's sixteen columns) are summed by halving: at distance 16 a lane keeps eight of its
// registers and takes its partner's sums of the same eight for the eight it hands over, at 8 four, at 4 two, at 2 one, and the last exchange at distance 1
// leaves both lanes of a pair with the sum of all 32 rows of register r = (lane >> 1) & 15 -- 16 shuffles of a double where 16 whole butterflies take 80, and
// one fixed tree per column.  The even lane of the pair writes it, one 8-byte store, to the column's slot; a column of an unselected block has no slot
// written (the finish kernel does not read it), a ragged column of a selected block gets +0.0.  Called by whole waves (the group loops are wave-uniform).
template <int N>
__device__ __forceinline__ void sd_halve(const double (&in)[2 * N], double (&out)[N], bool upper, int dist) {
#pragma unroll
    for (int j = 0; j < N; j++) {
        const double mine = upper ? in[j + N] : in[j], theirs = upper ? in[j] : in[j + N];
        out[j] = mine + __shfl_xor(theirs, dist);
    }
}

__device__ __forceinline__ void sd_score(const SddmmParams& p, const BlockRowDesc& br, const f32x16& acc, double* slots, int64_t q0, int64_t nq, int mt, int lane,
                                         const uint8_t* keep) {
    const int i = lane & 31;
    const int64_t cq = sd_column<true>(p, br, nq, q0 + i, keep);
    const unsigned long long live = __ballot(cq >= 0);
    const unsigned long long dead = __ballot(cq == -2);
    double s16[16], s8[8], s4[4], s2[2], s1[1];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int j = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const double d = (i < mt && ((live >> j) & 1)) ? (double)acc[r] : 0.0;
        s16[r] = d * d;
    }
    sd_halve<8>(s16, s8, (lane & 16) != 0, 16);
    sd_halve<4>(s8, s4, (lane & 8) != 0, 8);
    sd_halve<2>(s4, s2, (lane & 4) != 0, 4);
    sd_halve<1>(s2, s1, (lane & 2) != 0, 2);
    const double sum = s1[0] + __shfl_xor(s1[0], 1);
    const int r = i >> 1, j = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (!(lane & 1) && q0 + j < nq && !((dead >> j) & 1)) slots[q0 + j] = sum;
}

// the groups of an item.  LIVE: positions g0 .. g0 + 15 of the block-row's compacted list (ng = 0: the item has nothing to do); else g0 .. g0 + ng - 1
template <bool LIVE>
struct SdGroups {
    const int32_t* list;
    int g0, ng;
    __device__ __forceinline__ SdGroups(const SddmmItem& it, const SddmmLive& lv) : list(nullptr), g0(it.g0), ng(it.ng) {
        if constexpr (LIVE) {
            list = lv.groups + lv.goff[it.brow] + it.g0;
            ng = min(max(lv.count[it.brow] - it.g0, 0), kSdGroups);
        }
    }
    // group number of slot s (wave-uniform); LIVE: of slot min(s, ng - 1), ng >= 1 -- an unconditional load, so that a wave's four are issued together
    __device__ __forceinline__ int at(int s) const {
        if constexpr (LIVE) return list[min(s, ng - 1)];
        else return g0 + s;
    }
};

template <int MODE>
__device__ __forceinline__ void sddmm_f32_body(const SddmmParams& p, const SddmmLive& lv, const SddmmScore& sc) {
    constexpr bool LIVE = MODE != kSdPlain;
    __shared__ float xs[kKC32][32];
    const SddmmItem it = p.items[blockIdx.x];
    const SdGroups<LIVE> grp(it, lv);
    const BlockRowDesc br = p.brows[it.brow];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mt = min(32, br.h - it.r0);
    const int64_t nq = (int64_t)br.nb * p.w;
    if constexpr (LIVE)
        if (grp.ng == 0) return;                                        // (the whole workgroup, before the first barrier)
    const float* X = (const float*)p.X + (int64_t)br.c_row + it.r0;
    const float* Y = (const float*)p.Y;
    const float* yp[kSdGpw];
    bool ok[kSdGpw];
    int gq[kSdGpw];
#pragma unroll
    for (int t = 0; t < kSdGpw; t++) gq[t] = grp.at(wv + kSdWaves * t);
    int64_t colv[kSdGpw];
    if constexpr (LIVE) {
        int64_t qs[kSdGpw];
#pragma unroll
        for (int t = 0; t < kSdGpw; t++) {
            gq[t] = __builtin_amdgcn_readfirstlane(gq[t]);
            qs[t] = (int64_t)gq[t] * 32 + (lane & 31);
        }
        sd_columns_live<kSdGpw>(p, br, nq, qs, lv.keep, colv);
    }
#pragma unroll
    for (int t = 0; t < kSdGpw; t++) {
        const int64_t col = LIVE ? colv[t] : sd_column<false>(p, br, nq, (int64_t)gq[t] * 32 + (lane & 31), nullptr);
        ok[t] = col >= 0 && wv + kSdWaves * t < grp.ng;
        yp[t] = Y + (ok[t] ? col : 0) + (int64_t)(lane >> 5) * p.ldy;
    }
    f32x16 acc[kSdGpw];
#pragma unroll
    for (int t = 0; t < kSdGpw; t++)
        for (int r = 0; r < 16; r++) acc[t][r] = 0.0f;
    for (int n0 = 0; n0 < p.k; n0 += kKC32) {
        if (n0 > 0) __syncthreads();
#pragma unroll
        for (int e0 = 0; e0 < kKC32 * 32; e0 += kThreads) {
            const int e = e0 + tid, r = e & 31, nn = e >> 5;
            xs[nn][r] = (r < mt && n0 + nn < p.k) ? X[r + (int64_t)(n0 + nn) * p.ldx] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kSdGpw; t++) {
            if (wv + kSdWaves * t >= grp.ng) break;                     // wave-uniform
            float yv[kKC32 / 2];
#pragma unroll
            for (int s = 0; s < kKC32 / 2; s++) {
                const int n = n0 + 2 * s + (lane >> 5);
                yv[s] = (ok[t] && n < p.k) ? yp[t][(int64_t)(2 * s) * p.ldy] : 0.0f;
            }
            yp[t] += (int64_t)kKC32 * p.ldy;
#pragma unroll
            for (int s = 0; s < kKC32 / 2; s++)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(yv[s], xs[2 * s + (lane >> 5)][lane & 31], acc[t], 0, 0, 0);
        }
    }
    const int64_t base = br.a_off + it.r0;
#pragma unroll
    for (int t = 0; t < kSdGpw; t++) {
        if (wv + kSdWaves * t >= grp.ng) break;
        if constexpr (MODE == kSdScore) sd_score(p, br, acc[t], sc.slots + sc.soff[it.brow] + (int64_t)(it.r0 >> 5) * nq, (int64_t)gq[t] * 32, nq, mt, lane, lv.keep);
        else sd_store<LIVE>(p, br, acc[t], p.G, base, (int64_t)gq[t] * 32, nq, br.h, mt, lane, p.accumulate, lv.keep);
    }
}

__global__ __launch_bounds__(kThreads) void vbs_sddmm_f32_kernel(const SddmmParams p) { sddmm_f32_body<kSdPlain>(p, SddmmLive{}, SddmmScore{}); }
__global__ __launch_bounds__(kThreads) void vbs_sdlive_f32_kernel(const SddmmParams p, const SddmmLive lv) { sddmm_f32_body<kSdLive>(p, lv, SddmmScore{}); }

// 8 consecutive k (kb + 8 (lane >> 5) .. + 7) of entity lane & 31 from a [k][32] image of 16-bit values: two transposed reads.  Lane 4q + p of a
// 16-lane group addresses row kb + 8 (lane >> 5) + 4 t + q, entities 16 ((lane >> 4) & 1) + 4 p .. + 3; lane i of the group receives entity i.
// A 32-lane half reads 4 whole 64-byte rows: conflict-free.
__device__ __forceinline__ s16x8 sd_tr_frag(const uint16_t* img, int kb, int lane) {
    const int off = (kb + 8 * (lane >> 5) + ((lane & 15) >> 2)) * 32 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + off));
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + off + 4 * 32));
    return s16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

struct SdLds16 {
    uint16_t x[kKC16][32];                          // X tile of the chunk, [k][row]
    uint16_t y[kSdWaves][kSdGpw][kKC16][32];        // per wave and group: Y of the chunk, [k][stored column]
};

// VEC (w, ldy multiples of 8, Y 16-byte aligned): a run of 8 stored columns is 8 consecutive columns of Y, 16 aligned bytes -- one load per lane
// puts 8 columns of one k in the image (4 lanes a row of it); otherwise every lane gathers its own column, one 16-bit load per k
template <bool BF16, bool VEC, int MODE>
__device__ __forceinline__ void sddmm_h16_body(const SddmmParams& p, const SddmmLive& lv, const SddmmScore& sc) {
    constexpr bool LIVE = MODE != kSdPlain;
    __shared__ __attribute__((aligned(16))) SdLds16 lds;   // (the only LDS object: its base, and every row, is 16-byte aligned)
    const SddmmItem it = p.items[blockIdx.x];
    const SdGroups<LIVE> grp(it, lv);
    const BlockRowDesc br = p.brows[it.brow];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mt = min(32, br.h - it.r0);
    const int64_t nq = (int64_t)br.nb * p.w;
    if constexpr (LIVE)
        if (grp.ng == 0) return;                                        // (the whole workgroup, before the first barrier)
    const uint16_t* X = (const uint16_t*)p.X + (int64_t)br.c_row + it.r0;
    const uint16_t* Y = (const uint16_t*)p.Y;
    const uint16_t* yp[kSdGpw];
    bool ok[kSdGpw], full[kSdGpw];
    int gq[kSdGpw];
#pragma unroll
    for (int t = 0; t < kSdGpw; t++) gq[t] = grp.at(wv + kSdWaves * t);
    int64_t colv[kSdGpw];
    if constexpr (LIVE) {
        int64_t qs[kSdGpw];
#pragma unroll
        for (int t = 0; t < kSdGpw; t++) {
            gq[t] = __builtin_amdgcn_readfirstlane(gq[t]);
            qs[t] = (int64_t)gq[t] * 32 + (VEC ? 8 * (lane & 3) : lane & 31);
        }
        sd_columns_live<kSdGpw>(p, br, nq, qs, lv.keep, colv);
    }
#pragma unroll
    for (int t = 0; t < kSdGpw; t++) {
        const int64_t q0 = (int64_t)gq[t] * 32;
        const int64_t col = LIVE ? colv[t] : sd_column<false>(p, br, nq, VEC ? q0 + 8 * (lane & 3) : q0 + (lane & 31), nullptr);     // (VEC: w % 8 == 0, the 8 columns lie in one block)
        ok[t] = col >= 0 && wv + kSdWaves * t < grp.ng;
        yp[t] = Y + (ok[t] ? col : 0) + (int64_t)(VEC ? lane >> 2 : lane >> 5) * p.ldy;
        full[t] = ok[t] && col + 8 <= p.cols;
    }
    f32x16 acc[kSdGpw];
#pragma unroll
    for (int t = 0; t < kSdGpw; t++)
        for (int r = 0; r < 16; r++) acc[t][r] = 0.0f;
    for (int n0 = 0; n0 < p.k; n0 += kKC16) {
        if (n0 > 0) __syncthreads();
#pragma unroll
        for (int e0 = 0; e0 < kKC16 * 32; e0 += kThreads) {
            const int e = e0 + tid, r = e & 31, nn = e >> 5;
            lds.x[nn][r] = (r < mt && n0 + nn < p.k) ? X[r + (int64_t)(n0 + nn) * p.ldx] : (uint16_t)0;
        }
#pragma unroll
        for (int t = 0; t < kSdGpw; t++) {
            if (wv + kSdWaves * t >= grp.ng) break;
            if constexpr (VEC) {
#pragma unroll
                for (int s = 0; s < kKC16 / 16; s++) {
                    const int nn = (lane >> 2) + 16 * s;
                    const uint16_t* src = yp[t] + (int64_t)(n0 + 16 * s) * p.ldy;
                    u32x4 v = {0u, 0u, 0u, 0u};
                    if (full[t] && n0 + nn < p.k) v = *(const u32x4*)src;
                    else if (ok[t] && n0 + nn < p.k) {                  // the ragged last block column: 1..7 of the 8 columns exist
                        const int64_t col = (src - Y) % p.ldy;
#pragma unroll
                        for (int e = 0; e < 8; e++)
                            if (col + e < p.cols) v[e >> 1] |= (uint32_t)src[e] << (16 * (e & 1));
                    }
                    *(u32x4*)&lds.y[wv][t][nn][8 * (lane & 3)] = v;
                }
            } else {
#pragma unroll
                for (int s = 0; s < kKC16 / 2; s++) {
                    const int n = n0 + 2 * s + (lane >> 5);
                    lds.y[wv][t][2 * s + (lane >> 5)][lane & 31] = (ok[t] && n < p.k) ? yp[t][(int64_t)(n0 + 2 * s) * p.ldy] : (uint16_t)0;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < kKC16 / 16; m++) {
            const s16x8 xf = sd_tr_frag(&lds.x[0][0], 16 * m, lane);
#pragma unroll
            for (int t = 0; t < kSdGpw; t++) {
                if (wv + kSdWaves * t >= grp.ng) break;
                const s16x8 yf = sd_tr_frag(&lds.y[wv][t][0][0], 16 * m, lane);
                if constexpr (BF16) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, yf), __builtin_bit_cast(bf16x8, xf), acc[t], 0, 0, 0);
                else acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, yf), __builtin_bit_cast(f16x8, xf), acc[t], 0, 0, 0);
            }
        }
    }
    const int64_t base = br.a_off + it.r0;
#pragma unroll
    for (int t = 0; t < kSdGpw; t++) {
        if (wv + kSdWaves * t >= grp.ng) break;
        if constexpr (MODE == kSdScore) sd_score(p, br, acc[t], sc.slots + sc.soff[it.brow] + (int64_t)(it.r0 >> 5) * nq, (int64_t)gq[t] * 32, nq, mt, lane, lv.keep);
        else sd_store<LIVE>(p, br, acc[t], p.G, base, (int64_t)gq[t] * 32, nq, br.h, mt, lane, p.accumulate, lv.keep);
    }
}

template <bool BF16, bool VEC>
__global__ __launch_bounds__(kThreads) void vbs_sddmm_h16_kernel(const SddmmParams p) { sddmm_h16_body<BF16, VEC, kSdPlain>(p, SddmmLive{}, SddmmScore{}); }
template <bool BF16, bool VEC>
__global__ __launch_bounds__(kThreads) void vbs_sdlive_h16_kernel(const SddmmParams p, const SddmmLive lv) { sddmm_h16_body<BF16, VEC, kSdLive>(p, lv, SddmmScore{}); }
// the score forms (sparta_vbs_sddmm_block_ssq), behind the ten kernels above: the same bodies up to the end of a group, where sd_score stands for sd_store
__global__ __launch_bounds__(kThreads) void vbs_sdscore_f32_kernel(const SddmmParams p, const SddmmLive lv, const SddmmScore sc) { sddmm_f32_body<kSdScore>(p, lv, sc); }
template <bool BF16, bool VEC>
__global__ __launch_bounds__(kThreads) void vbs_sdscore_h16_kernel(const SddmmParams p, const SddmmLive lv, const SddmmScore sc) {
    sddmm_h16_body<BF16, VEC, kSdScore>(p, lv, sc);
}

// one wave per block, kPruneWaves blocks per workgroup (as k_prune.hip): an unselected block (per the snapshot) scores +0.0 and reads nothing; otherwise lane l
// takes the block's slots l, l + 64, ... in the order tile by tile, column by column, and the lanes are summed by xor-shuffle.  No LDS, no barrier, no atomics.
__global__ __launch_bounds__(kThreads) void vbs_sdscore_finish_kernel(const ScoreBlock* __restrict__ blocks, int64_t n_blocks, int w, const uint8_t* __restrict__ snap,
                                                                     const double* __restrict__ slots, double* __restrict__ ssq_out) {
    const int64_t b = (int64_t)blockIdx.x * kPruneWaves + (threadIdx.x >> 6);
    if (b >= n_blocks) return;                  // (the whole wave)
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    if (snap[b] != 0) {                         // (the whole wave)
        const ScoreBlock blk = blocks[b];
        const int64_t n = (int64_t)blk.ntiles * w;
        for (int64_t e = lane; e < n; e += 64) {
            const int64_t t = e / w, c = e - t * w;
            s += slots[blk.slot0 + t * blk.tstride + c];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) ssq_out[b] = s;
}

}  // namespace

void launch_sddmm(int dtype, unsigned n_items, hipStream_t st, const SddmmParams& p) {
    if (n_items == 0) return;
    const bool vec = p.w % 8 == 0 && p.ldy % 8 == 0 && (uintptr_t)p.Y % 16 == 0;
    if (dtype == SPARTA_F32) hipLaunchKernelGGL(vbs_sddmm_f32_kernel, dim3(n_items), dim3(kThreads), 0, st, p);
    else if (dtype == SPARTA_BF16 && vec) hipLaunchKernelGGL((vbs_sddmm_h16_kernel<true, true>), dim3(n_items), dim3(kThreads), 0, st, p);
    else if (dtype == SPARTA_BF16) hipLaunchKernelGGL((vbs_sddmm_h16_kernel<true, false>), dim3(n_items), dim3(kThreads), 0, st, p);
    else if (vec) hipLaunchKernelGGL((vbs_sddmm_h16_kernel<false, true>), dim3(n_items), dim3(kThreads), 0, st, p);
    else hipLaunchKernelGGL((vbs_sddmm_h16_kernel<false, false>), dim3(n_items), dim3(kThreads), 0, st, p);
}

void launch_sddmm_live(int dtype, unsigned n_items, hipStream_t st, const SddmmParams& p, const SddmmLive& lv) {
    if (n_items == 0) return;
    const bool vec = p.w % 8 == 0 && p.ldy % 8 == 0 && (uintptr_t)p.Y % 16 == 0;
    if (dtype == SPARTA_F32) hipLaunchKernelGGL(vbs_sdlive_f32_kernel, dim3(n_items), dim3(kThreads), 0, st, p, lv);
    else if (dtype == SPARTA_BF16 && vec) hipLaunchKernelGGL((vbs_sdlive_h16_kernel<true, true>), dim3(n_items), dim3(kThreads), 0, st, p, lv);
    else if (dtype == SPARTA_BF16) hipLaunchKernelGGL((vbs_sdlive_h16_kernel<true, false>), dim3(n_items), dim3(kThreads), 0, st, p, lv);
    else if (vec) hipLaunchKernelGGL((vbs_sdlive_h16_kernel<false, true>), dim3(n_items), dim3(kThreads), 0, st, p, lv);
    else hipLaunchKernelGGL((vbs_sdlive_h16_kernel<false, false>), dim3(n_items), dim3(kThreads), 0, st, p, lv);
}

void launch_sddmm_score(int dtype, unsigned n_items, hipStream_t st, const SddmmParams& p, const SddmmLive& lv, const SddmmScore& sc) {
    if (n_items == 0) return;
    const bool vec = p.w % 8 == 0 && p.ldy % 8 == 0 && (uintptr_t)p.Y % 16 == 0;
    if (dtype == SPARTA_F32) hipLaunchKernelGGL(vbs_sdscore_f32_kernel, dim3(n_items), dim3(kThreads), 0, st, p, lv, sc);
    else if (dtype == SPARTA_BF16 && vec) hipLaunchKernelGGL((vbs_sdscore_h16_kernel<true, true>), dim3(n_items), dim3(kThreads), 0, st, p, lv, sc);
    else if (dtype == SPARTA_BF16) hipLaunchKernelGGL((vbs_sdscore_h16_kernel<true, false>), dim3(n_items), dim3(kThreads), 0, st, p, lv, sc);
    else if (vec) hipLaunchKernelGGL((vbs_sdscore_h16_kernel<false, true>), dim3(n_items), dim3(kThreads), 0, st, p, lv, sc);
    else hipLaunchKernelGGL((vbs_sdscore_h16_kernel<false, false>), dim3(n_items), dim3(kThreads), 0, st, p, lv, sc);
}

void launch_sddmm_score_finish(hipStream_t st, const ScoreBlock* blocks, int64_t n_blocks, int w, const uint8_t* snap, const double* slots, double* ssq) {
    if (n_blocks == 0) return;
    hipLaunchKernelGGL(vbs_sdscore_finish_kernel, dim3((unsigned)((n_blocks + kPruneWaves - 1) / kPruneWaves)), dim3(kThreads), 0, st, blocks, n_blocks, w, snap, slots, ssq);
}

}  // namespace sparta_dev
