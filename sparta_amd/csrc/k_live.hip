// k_live.hip -- the live-block set of a VBS handle (sparta_vbs_set_live_blocks, include/sparta_amd.h): from the caller's keep[n_blocks] the snapshot the
// handle holds and the compacted lists the two backward products walk.  Pattern-only inputs (block-row descriptors, the block-column index, the map list
// position -> block number) are the handle's; nothing of its images is read or written.
//   vbs_live_groups_kernel     per block-row the numbers of its live groups of 32 stored columns, compacted, and their count; the snapshot of keep
//   vbs_live_columns_kernel    per block column its live SpmmTBlock records and block numbers, compacted, and the items with l1 = l0 + live count
// and, further down, the word kernel of the live steps and the compaction of the step records for the live forward product (vbs_fwdlive_compact_kernel).
// One WAVE per block-row / block column, kLiveWaves per workgroup, as k_prune.hip: a wave walks its list 64 entries at a time, a ballot of the live entries
// and the count of the set bits below the lane give every live entry its place behind the ones already written.  Stable (list order is kept), no atomics,
// no LDS, no barrier, one fixed order: the lists are a function of keep alone.  Every position of every output slice is written on every call (-1 / a zero
// record behind the live entries), so nothing of an earlier mask is left.
#include "vbs_kernel_common.hpp"

namespace sparta_dev {
namespace {

constexpr int kLiveWaves = kThreads / 64;

// live entries in front of this lane
__device__ __forceinline__ int lv_prefix(unsigned long long mask) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u)); }

// wave wi: blocks 64 wi .. 64 wi + 63 of the snapshot, and block-row wi of the handle (brows holds the block-rows of height > 0; block b of one is block
// jab_off + b of the handle).  Group g covers stored columns 32 g .. 32 g + 31 of the block-row's nb * w: blocks 32 g / w .. min(32 g + 31, nb w - 1) / w.
__global__ __launch_bounds__(kThreads) void vbs_live_groups_kernel(const BlockRowDesc* __restrict__ brows, int64_t n_brows, int w, const uint8_t* __restrict__ keep,
                                                                 int64_t n_blocks, uint8_t* __restrict__ snap, const int32_t* __restrict__ goff, int32_t* __restrict__ groups,
                                                                 int32_t* __restrict__ count) {
    const int64_t wi = (int64_t)blockIdx.x * kLiveWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t sb = wi * 64 + lane;
    if (sb < n_blocks) snap[sb] = keep[sb] != 0 ? 1 : 0;
    if (wi >= n_brows) return;                  // (the whole wave)
    const BlockRowDesc br = brows[wi];
    const int64_t nq = (int64_t)br.nb * w;
    const int ng = (int)((nq + 31) / 32);
    const uint8_t* kb = keep + br.jab_off;
    int32_t* out = groups + goff[wi];
    int n = 0;
    for (int g0 = 0; g0 < ng; g0 += 64) {       // (wave-uniform trip count: the ballot sees all 64 lanes)
        const int g = g0 + lane;
        bool live = false;
        if (g < ng) {
            const int64_t q_hi = min((int64_t)32 * g + 31, nq - 1);
            for (int64_t b = (int64_t)32 * g / w; b <= q_hi / w; b++) live = live || kb[b] != 0;
        }
        const unsigned long long mask = __ballot(live);
        if (live) out[n + lv_prefix(mask)] = g;
        n += __popcll(mask);
    }
    for (int i = n + lane; i < ng; i += 64) out[i] = -1;
    if (lane == 0) count[wi] = n;
}

// wave jb: block column jb.  Its items (one per panel of 32 stored columns) share one list blocks[l0, l1).
__global__ __launch_bounds__(kThreads) void vbs_live_columns_kernel(const SpmmTItem* __restrict__ items, const SpmmTBlock* __restrict__ blocks, const int32_t* __restrict__ tmap,
                                                                  int64_t block_cols, int panels, const uint8_t* __restrict__ keep, SpmmTItem* __restrict__ live_items,
                                                                  SpmmTBlock* __restrict__ live_blocks, int32_t* __restrict__ live_ids, int32_t* __restrict__ live_count) {
    const int64_t jb = (int64_t)blockIdx.x * kLiveWaves + (threadIdx.x >> 6);
    if (jb >= block_cols) return;               // (the whole wave)
    const int lane = threadIdx.x & 63;
    const SpmmTItem first = items[jb * panels];
    const int l0 = first.l0, l1 = first.l1;
    int n = 0;
    for (int base = l0; base < l1; base += 64) {
        const int l = base + lane;
        const int blk = l < l1 ? tmap[l] : 0;
        const bool live = l < l1 && keep[blk] != 0;
        const unsigned long long mask = __ballot(live);
        if (live) {
            const int pos = l0 + n + lv_prefix(mask);
            live_blocks[pos] = blocks[l];
            live_ids[pos] = blk;
        }
        n += __popcll(mask);
    }
    for (int l = l0 + n + lane; l < l1; l += 64) {
        live_blocks[l] = SpmmTBlock{0, 0, 0};
        live_ids[l] = -1;
    }
    for (int pn = lane; pn < panels; pn += 64) {
        SpmmTItem it = items[jb * panels + pn];
        it.l1 = l0 + n;
        live_items[jb * panels + pn] = it;
    }
    if (lane == 0) live_count[jb] = n;
}

// The live words of the image kernels of the steps (sparta_vbs_set_live_steps; k_update_image.inc reads them): word i belongs to one step of the fp32 one-tile
// plan / to rows 0..31 / rows 32..63 of one 16-bit slice, and wmap[i] is the number of the block that step / half lies in (pattern only, built next to
// build_live_maps; -1: a half the slice does not have).  A step is 32 columns of ONE block and a slice half kp columns of one block (the planner cuts blocks,
// whose width is a multiple of 32 wherever an image kernel exists), so all 32 column bits of a word are equal: all ones if the block is live in the snapshot,
// else zero.  One thread per word, a grid-stride loop, plain 4-byte vector stores, every word written on every call; no atomics, no LDS.  (The name avoids
// "vbs_live_": the tests count the two compaction kernels by it.)
__global__ __launch_bounds__(kThreads) void vbs_lvstep_words_kernel(const int32_t* __restrict__ wmap, int64_t n_words, const uint8_t* __restrict__ snap,
                                                                  uint32_t* __restrict__ words) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_words; i += stride) {
        const int32_t b = wmap[i];
        words[i] = (b >= 0 && snap[b] != 0) ? 0xffffffffu : 0u;
    }
}

// Live forward (sparta_vbs_set_live_forward): the rule of live_forward_compact_host (vbs_plan.cpp) on the device.  One WAVE per range of one stream image:
// it walks the range segment by segment (seg_last[q], pattern only, says where the segment of step q ends), 64 steps at a time; a step's two live bits are
// the two live words of its slice.  A first pass counts the kept steps of the range (the dropped ones go behind ALL of them), the second pass counts the
// live steps of a segment, then writes: kept records, edited, to the front in order, dropped records unchanged behind them in order.  Ballot + mbcnt give the
// places; no atomics, no LDS, no barrier.  Every position of the range and its live range are written on every call.  Reads the plain records, writes the
// second array: the plain arrays are never written.  (The name avoids "vbs_live_": the tests count the two compaction kernels above by it.)
__global__ __launch_bounds__(kThreads) void vbs_fwdlive_compact_kernel(const StepRec* __restrict__ steps, const int32_t* __restrict__ seg_last, const int32_t* __restrict__ ranges,
                                                                     int64_t n_ranges, const uint32_t* __restrict__ words, int pair, StepRec* __restrict__ out,
                                                                     int32_t* __restrict__ ranges_out) {
    const int64_t r = (int64_t)blockIdx.x * kLiveWaves + (threadIdx.x >> 6);
    if (r >= n_ranges) return;                  // (the whole wave)
    const int lane = threadIdx.x & 63;
    const int b = ranges[2 * r], e = ranges[2 * r + 1];
    // a record as two 16-byte halves: x = {a_off (two words), b_row, h}, y = {c_row, mt_flags, slot, pad}
    const int4* __restrict__ in4 = reinterpret_cast<const int4*>(steps);
    int4* __restrict__ out4 = reinterpret_cast<int4*>(out);
    // the halves of step s that are present and live: bit 0 rows 0..31, bit 1 rows 32..63
    auto halves = [&](int s, int32_t flags) -> int {
        const int lo = (!pair || !(flags & STEP_LO_ABSENT)) && words[2 * (int64_t)s] != 0u;
        const int hi = pair && !(flags & STEP_HI_ABSENT) && words[2 * (int64_t)s + 1] != 0u;
        return lo | (hi << 1);
    };
    // the end of the segment that starts at q (wave-uniform; clamped into the range, so that the walk ends whatever the map holds)
    auto segment_end = [&](int q) { return min(max(__builtin_amdgcn_readfirstlane(seg_last[q]), q), e - 1); };
    auto count_live = [&](int q, int sl) {
        int n = 0;
        for (int s0 = q; s0 <= sl; s0 += 64) {  // (wave-uniform trip count: the ballot sees all 64 lanes)
            const int s = s0 + lane;
            const int hv = s <= sl ? halves(s, steps[s].mt_flags) : 0;
            n += __popcll(__ballot(hv != 0));
        }
        return n;
    };
    int kept_total = 0;
    for (int q = b; q < e;) {
        const int sl = segment_end(q);
        const int n = count_live(q, sl);
        kept_total += n > 0 ? n : 1;
        q = sl + 1;
    }
    int nk = 0, nd = 0;
    for (int q = b; q < e;) {
        const int sl = segment_end(q);
        const int n = count_live(q, sl);
        const int4 last = in4[2 * (int64_t)sl + 1];                  // the epilogue fields of the segment: c_row, mt_flags, slot
        int seen = 0;
        for (int s0 = q; s0 <= sl; s0 += 64) {
            const int s = s0 + lane;
            const bool in = s <= sl;
            const int4 x = in4[2 * (int64_t)(in ? s : sl)];
            int4 y = in4[2 * (int64_t)(in ? s : sl) + 1];
            const int hv = in ? halves(s, y.y) : 0;
            const bool lv = hv != 0;
            const bool keep = lv || (in && n == 0 && s == q);
            const unsigned long long m_live = __ballot(lv), m_keep = __ballot(keep), m_drop = __ballot(in && !keep);
            int64_t at = -1;
            if (keep) {
                const int idx = seen + lv_prefix(m_live);           // the step's place among the live steps of its segment
                const bool is_first = n == 0 || idx == 0, is_last = n == 0 || idx == n - 1;
                int32_t f = y.y & ~(STEP_FIRST | STEP_LAST | STEP_SPLIT);
                if (is_first) f |= STEP_FIRST;
                if (is_last) {
                    f = (f & ~0xffff) | (last.y & 0xffff) | STEP_LAST | (last.y & STEP_SPLIT);
                    y.x = last.x;
                    y.z = last.z;
                }
                if (!(hv & 1)) f |= STEP_LO_ABSENT;
                if (pair && !(hv & 2)) f |= STEP_HI_ABSENT;
                y.y = f;
                at = (int64_t)b + nk + lv_prefix(m_keep);
            } else if (in) {
                at = (int64_t)b + kept_total + nd + lv_prefix(m_drop);
            }
            if (at >= 0) { out4[2 * at] = x; out4[2 * at + 1] = y; }
            seen += __popcll(m_live);
            nk += __popcll(m_keep);
            nd += __popcll(m_drop);
        }
        q = sl + 1;
    }
    if (lane == 0) { ranges_out[2 * r] = b; ranges_out[2 * r + 1] = b + kept_total; }
}

unsigned live_grid(int64_t waves) { return (unsigned)((waves + kLiveWaves - 1) / kLiveWaves); }

}  // namespace

void launch_live_step_words(hipStream_t st, const int32_t* wmap, int64_t n_words, const uint8_t* snap, uint32_t* words) {
    if (n_words <= 0) return;
    const int64_t groups = (n_words + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(vbs_lvstep_words_kernel, dim3((unsigned)std::min<int64_t>(groups, 65536)), dim3(kThreads), 0, st, wmap, n_words, snap, words);
}

void launch_live_forward_compact(hipStream_t st, const StepRec* steps, const int32_t* seg_last, const int32_t* ranges, int64_t n_ranges, const uint32_t* words, bool pair,
                                 StepRec* out, int32_t* ranges_out) {
    if (n_ranges <= 0) return;
    hipLaunchKernelGGL(vbs_fwdlive_compact_kernel, dim3(live_grid(n_ranges)), dim3(kThreads), 0, st, steps, seg_last, ranges, n_ranges, words, pair ? 1 : 0, out, ranges_out);
}

void launch_live_sddmm(hipStream_t st,const BlockRowDesc* brows, int64_t n_brows, int w, const uint8_t* keep, int64_t n_blocks, uint8_t* snap, const int32_t* goff,
                       int32_t* groups, int32_t* count) {
    const int64_t waves = std::max(n_brows, (n_blocks + 63) / 64);
    if (waves == 0) return;
    hipLaunchKernelGGL(vbs_live_groups_kernel, dim3(live_grid(waves)), dim3(kThreads), 0, st, brows, n_brows, w, keep, n_blocks, snap, goff, groups, count);
}

void launch_live_spmm_t(hipStream_t st, const SpmmTItem* items, const SpmmTBlock* blocks, const int32_t* tmap, int64_t block_cols, int panels, const uint8_t* keep,
                        SpmmTItem* live_items, SpmmTBlock* live_blocks, int32_t* live_ids, int32_t* live_count) {
    if (block_cols == 0) return;
    hipLaunchKernelGGL(vbs_live_columns_kernel, dim3(live_grid(block_cols)), dim3(kThreads), 0, st, items, blocks, tmap, block_cols, panels, keep, live_items, live_blocks,
                       live_ids, live_count);
}

}  // namespace sparta_dev
