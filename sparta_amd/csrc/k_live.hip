// k_live.hip -- the live-block set of a VBS handle (sparta_vbs_set_live_blocks, include/sparta_amd.h): from the caller's keep[n_blocks] the snapshot the
// handle holds and the compacted lists the two backward products walk.  Pattern-only inputs (block-row descriptors, the block-column index, the map list
// position -> block number) are the handle's; nothing of its images is read or written.
//   vbs_live_groups_kernel     per block-row the numbers of its live groups of 32 stored columns, compacted, and their count; the snapshot of keep
//   vbs_live_columns_kernel    per block column its live SpmmTBlock records and block numbers, compacted, and the items with l1 = l0 + live count
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

unsigned live_grid(int64_t waves) { return (unsigned)((waves + kLiveWaves - 1) / kLiveWaves); }

}  // namespace

void launch_live_step_words(hipStream_t st, const int32_t* wmap, int64_t n_words, const uint8_t* snap, uint32_t* words) {
    if (n_words <= 0) return;
    const int64_t groups = (n_words + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(vbs_lvstep_words_kernel, dim3((unsigned)std::min<int64_t>(groups, 65536)), dim3(kThreads), 0, st, wmap, n_words, snap, words);
}

void launch_live_sddmm(hipStream_t st, const BlockRowDesc* brows, int64_t n_brows, int w, const uint8_t* keep, int64_t n_blocks, uint8_t* snap, const int32_t* goff,
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
