// vbs_device.hpp -- declarations shared by the translation units of the device side of libsparta_amd.so:
//   k_f32_class.hip   per-class fp32 MFMA kernels + the exact-order parity kernel
//   k_f32_stream.hip  persistent fp32 stream kernels, fix-up, B-tail copy, zero fill
//   k_f32_direct.hip  the no-barrier fp32 kernel of the one-tile plan (one block per step)
//   k_f32_packed.hip  ... and its packed form (partly empty blocks of a tile share a step)
//   k_h16.hip         fp16 / bf16 storage: LDS-staged and direct stream kernels, conversions (the direct kernel's body: k_h16_direct.inc)
//   k_h16_live.hip    the live form of the direct 16-bit kernel: the same body on the compacted records of sparta_vbs_set_live_forward
//   k_h16_a8.hip      the a8 form of the direct 16-bit kernel (fp8 e4m3 image of A, sparta_vbs_set_forward_a8) and the kernel that quantises the image
//   k_h16_a8_live.hip the a8 form on the compacted records of live forward (sparta_vbs_set_a8_live) and the kernel that places the exponent words there
//   k_hub16.hip       the GEMM-shaped kernel for the hub plan of 16-bit handles (the dense part under the fixed 64 x 64 grid)
//   k_sparse.hip      sparse-row kernels, layout transposes, row-block pack
//   k_colres.hip      the resident-column product: small fp32 handles whose rows are all sparse rows, columns of B held in LDS
//   k_union.hip       the MFMA kernels of the column-compacted ("union-pattern") tiles, fp32 and 16-bit
//   k_sddmm.hip       sampled dense-dense product on a handle's stored blocks (sparta_vbs_sddmm) and its score form (sparta_vbs_sddmm_block_ssq)
//   k_spmm_t.hip      the transposed product on a handle's own stored blocks (sparta_vbs_spmm_t)
//   k_update.hip      new values for the images of an updatable handle (sparta_vbs_set_values) and the optimizer steps (sparta_vbs_sgd_step, sparta_vbs_adam_step)
//   k_gradctl.hip     the control record of gradient clipping and loss scaling (sparta_grad_stats, sparta_grad_ctl_finish)
//   k_prune.hip       block pruning: per-block sums of squares, zero fill of chosen blocks (sparta_vbs_block_ssq, sparta_vbs_mask_blocks)
//   k_epilogue.hip    the epilogue of a linear layer: bias, activation, output type, bias gradient (sparta_epilogue_fwd, sparta_epilogue_bwd)
//   k_live.hip        the live-block set of a handle: stable compaction of the lists sddmm and spmm_t walk (sparta_vbs_set_live_blocks)
//   k_repattern.hip   values and optimizer state moved from one handle's layout to another's (sparta_vbs_move_blocks)
//   k_dense.hip       a dense matrix and the stored blocks of a handle: block scores, gather, scatter (sparta_dense_block_ssq, sparta_vbs_gather_dense / _scatter_dense)
//   vbs_plan.cpp      host: stream plans (step lists, worker ranges, split tiles), hub plan, packed plan, block table
//   vbs_union.cpp     host: the device form of the column-compacted tiles
//   vbs_capi.cpp      host: device image (sparta_vbs) and the sparta_vbs_* entries that make HIP calls: create, the products, the training steps, pruning, the live set
//   vbs_host_check.cpp host: the entries that make no HIP call (sparta_*_host_check, sparta_vbs_*_host, the packing and quantising rules)
//   vbs_epilogue.cpp  host: sparta_epilogue_fwd / _bwd / _scratch_bytes
//   (vbs_host.hpp: what the files of the entry points share among themselves; the other host files -- capi.cpp, reorder.cpp, vbs_build.cpp, io.cpp -- see host_core.hpp only)
// Every kernel TU exports plain launch functions (namespace sparta_dev); the host TUs never see a __global__ symbol.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <memory>
#include <vector>

#include "host_core.hpp"

namespace sparta_dev {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 4-byte aligned: global_load_dwordx4 on any float address
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr int kTN = 128;   // columns of C per workgroup
constexpr int kKP = 64;    // k-depth of one panel step

// one row tile of one block-row
struct TileDesc {
    int64_t a_off;     // element offset into A of (first block of the block-row) + r0
    int64_t jab_off;   // offset into jab of the block-row's first block-column id
    int32_t nb;        // nonzero blocks in the block-row
    int32_t h;         // block-row height = leading dimension of each of its blocks
    int32_t c_row;     // first row of C written by this tile
    int32_t mt_flags;  // low 16 bits: rows in this tile (<= class height); TILE_* flags above
};
constexpr int32_t TILE_TAIL = 1 << 16;   // the block-row's last block lies in the zero-padded last block column (cols % w != 0)
static_assert(sizeof(TileDesc) == 32, "TileDesc must stay 32 bytes");

struct SpmmParams {
    const TileDesc* tiles;
    const int32_t* jab;
    const float* A;
    const float* B;
    float* C;
    int64_t ldb, ldc;
    int64_t cols;      // valid rows of B
    int32_t n_tiles, n_ntiles;
    int32_t N, w;
    int32_t b_row_major, c_row_major;
    int32_t accumulate, vec_ok;
    int64_t shard_stride; // elements between consecutive slabs of a gathered B
    int64_t shard_rows;   // 0: B is one matrix; >0: B is an all-gather result of column-major shard_rows x N slabs
    long long* clk;       // clock probe (NULL = off): workgroup 0 writes {s_memtime, s_memrealtime} at entry and exit
};

constexpr int SK_KP = 32;                 // k depth of a step
constexpr int SK_TM = 64;                 // max rows of a tile
constexpr int32_t STEP_FIRST = 1 << 16;   // first step of a (segment of a) tile: accumulators start at zero
constexpr int32_t STEP_LAST = 1 << 17;    // last step of a (segment of a) tile: run the epilogue
constexpr int32_t STEP_SPLIT = 1 << 18;   // the tile is shared with another worker: epilogue goes to the workspace
constexpr int32_t STEP_LO_ABSENT = 1 << 27;  // 16-bit pair tiles (two vertically adjacent 32-row block-rows walked as ONE 64-row tile over the union of their block
constexpr int32_t STEP_HI_ABSENT = 1 << 28;  // columns, vbs_plan.cpp): the lower / upper block-row has no block in this step's column -- that half of the slice is zeros and is not fetched
constexpr int32_t STEP_KPAIRS_SHIFT = 24;  // bits 24..26: (MFMA pairs this step needs) - 1, fp32 one-tile plans with a fragment image (k-compaction: the
                                           // non-empty columns of the step's slice of A come first, vbs_plan.cpp); read by vbs_spmm_f32_direct_kernel only
constexpr int64_t kAFragSlice = 1040;      // floats per step of the fragment image: 16 (the step's LDS position table: 32 bytes + padding) + 1024 (fragments)
constexpr int32_t STEP_TAIL = 1 << 19;    // panel of the zero-padded last block column: read from StreamParams::B_tail, b_row = k offset in it
constexpr int SK_SLOT_FLOATS = 32 * kThreads;   // one partial accumulator image: 32 registers x 256 threads

struct StepRec {                          // 32 bytes, one per (block, 32-deep k slice), in execution order
    int64_t a_off;                        // element offset into A of (tile row 0, first k of this step)
    int32_t b_row;                        // first row of B of this step's panel (jb * w + ks)
    int32_t h;                            // leading dimension of the A block (block-row height)
    int32_t c_row;                        // first row of C of the tile
    int32_t mt_flags;                     // rows of the tile (low 16 bits) | STEP_* flags
    int32_t slot;                         // workspace slot for STEP_LAST|STEP_SPLIT, else -1
    int32_t pad;                          // gathered-B step lists: index of the slab that holds b_row (b_row is then slab-local); else 0
};
static_assert(sizeof(StepRec) == 32, "StepRec must stay 32 bytes");

struct FixRec {                           // one per split tile
    int32_t c_row, mt;
    int32_t slot_begin, n_slots;          // its partial images: fix_slots[slot_begin .. slot_begin + n_slots)
};

// packed plan of fp32 handles (vbs_plan.cpp, k_f32_packed.hip)
constexpr int32_t kPackNoRow = 0x20000000;                // table entry of an unused slot: 4 x this is past the end of every descriptor of B
constexpr int kPackPadSlices = 8;                         // slices behind the end of the packed image (the pipeline requests tables five steps ahead)
struct PackLoc { int32_t step; int32_t slot0_mask; };     // per block of the one-tile plan: its packed step; slot0 | mask << 8

struct StreamParams {
    const StepRec* steps;
    const int32_t* worker_range;          // [2 * P]: begin, end step of every worker
    const float* A;
    const float* B;
    const float* B_tail;                  // zero-padded copy of B's last (partial) block row: w x N, ld = w (col-major) / N (row-major)
    float* C;
    float* ws;                            // partial images: [n_ntiles][n_slots][SK_SLOT_FLOATS], one per segment of a split tile
    int64_t ldb, ldc, cols;
    int64_t shard_rows, shard_stride;
    int64_t ws_slab_stride;               // floats between the workspaces of consecutive 128-column slabs
    int32_t accumulate, c_row_major;
    int32_t N, w;
    long long* clk;                       // clock probe, see clock_probe()
    int32_t c_nt;                         // 1: non-temporal C stores (long tiles), 0: default cache policy (short tiles); see vbs_kernel_common.hpp
    int32_t stagger;                      // developer knob (SPARTA_STAGGER): workgroups of the second half of the grid start this many x 64 cycles late
    int32_t sub_ranges = 0;               // 1: worker_range holds two adjacent sub-worker ranges per workgroup (16-bit `wide16` plans)
};

// ---- the GEMM-shaped hub kernel of 16-bit handles (k_hub16.hip): group tiles of G = 2 or 4 sub-tiles of <= 64 rows (block-rows of the fixed 64 x 64 grid that
// share most of their block columns -- not necessarily neighbours), walked over the UNION of their block columns; a workgroup owns the group's rows x one
// 256-column slab of C and stages A and B once through LDS for all its waves
constexpr int kHubGMax = 4;               // most 64-row sub-tiles per group tile (the kernel has a two- and a four-sub-tile form)
struct HubStep {                          // 32 bytes, one per (group tile, KP-deep k slice), in execution order
    uint32_t a_lo, a_hi;                  // element offset into the 16-bit image of A of this step's first PRESENT slice (present slices back to back)
    int32_t b_row;                        // first row of B of the step's panel (row inside its slab for a gathered B; k offset into B_tail for STEP_TAIL)
    int32_t shard;                        // gathered B: index of the slab that holds b_row; else 0
    int32_t flags;                        // bits 0..3: which sub-tiles have a block in this block column; STEP_LAST / STEP_SPLIT / STEP_TAIL
    int32_t slot;                         // STEP_LAST | STEP_SPLIT: first of the segment's G consecutive workspace images (one per sub-tile), else -1
    int32_t tile;                         // index into HubTile
    int32_t pad;
};
static_assert(sizeof(HubStep) == 32, "HubStep must stay 32 bytes");
struct HubTile { int32_t c_row[4]; int32_t mt[4]; };      // per sub-tile: first row of C, rows (<= 64; 0: no such sub-tile)
struct HubParams {
    const HubStep* steps;
    const int32_t* worker_range;          // [2 * n_workers]: begin, end step of every worker
    const HubTile* tiles;
    const uint16_t* A;                    // slices of 64 rows x KP, [row][16-byte chunk c ^ swizzle(row)] (the LDS image, see k_hub16.hip)
    const uint16_t* B;
    const uint16_t* B_tail;               // zero-padded copy of B's last (partial) block row: w x N, ld = w; or nullptr
    float* C;
    float* ws;                            // partial images, as StreamParams::ws
    int64_t ldb, ldc;
    int64_t shard_stride;
    int64_t ws_slab_stride;               // floats between the workspaces of consecutive 128-column slabs
    int32_t accumulate, c_row_major, c_nt, w;
    int32_t n_slabs;                      // 256-column slabs of this launch: grid = n_workers x n_slabs workgroups (the slabs of a worker adjacent on one XCD)
    int32_t n_workers;
    int32_t n_cols;                       // columns of B / C (a multiple of 128): the last slab may be a half slab
    int32_t pad0;
};

constexpr int kFixGroup = 16;   // partial images per group of the fix-up group stage (k_f32_stream.hip)

struct SparseParams {
    const int64_t* rowptr;     // [n_rows + 1] into col / val
    const int32_t* col;
    const float* val;
    const int32_t* crow;       // C row of every sparse row
    const int32_t* list;       // the rows this launch handles (ordinals)
    int32_t n_list;
    const void* B;             // row-major, ld = ldb elements; fp32 (BK = 0), fp16 (1) or bf16 (2)
    int64_t b_col_stride;      // 0: row-major B as above.  > 0: B is COLUMN-major (element (k, n) at slab(k) + k % shard_rows + n * b_col_stride),
    int64_t shard_rows, shard_stride;   //      read in place, one 4-byte gather per element: only worth it for a handful of sparse rows
    int64_t ldb;
    float* out;                // out_is_c 1: row-major C (ld = ldc, row = crow); 2: COLUMN-major C (ld = ldc)
    int64_t ldo;
    int32_t out_is_c, accumulate, N;
    int32_t scalar_gather;     // 1: (column, value) pairs through scalar loads, row base in SGPRs (k_sparse.hip: sparse_row_partial_s); 0: the round-3 gather (SPARTA_SP_SCALAR=0)
};

// resident-column product (k_colres.hip): A as slots (rows, the long ones cut into chunks) sorted by length, 64 to a slice, entry k of a slice's slots contiguous
constexpr int kColresWaves = 16;        // waves of a workgroup of k_colres.hip (host layout and kernel agree on it)
struct ColresLong { int32_t row, first, n, pad; };   // a row cut into chunks: its cell in the staging image, the first of its extra cells, how many
// A matrix whose columns of B or of C do not fit LDS whole is cut: the rows of C into PARTS (a workgroup owns NC columns of one part: grid y), the columns of A into K RANGES (a workgroup
// walks them one after the other, its sums staying in registers: the rows of B of a range in LDS at a time).
constexpr int kColresMaxParts = 4, kColresMaxRanges = 4;
constexpr int kColresCellsPerPlane = 160 * 1024 / 4;      // floats of LDS: the most cells a column's staging image can have
struct ColresPartDev {
    int32_t r0, rows;          // the part's rows of C: [r0, r0 + rows), r0 a multiple of 4
    int32_t n_slices, n_long;
    int32_t plane;             // cells per column of the staging image (rows + extra cells, a multiple of 4)
    int32_t meta;              // offset (int32) of the part's block in `meta`: wslice[17], woff[n_ranges][17], bnd[n_ranges][n_slices]
    int32_t dest;              // offset (int32) of its dest[64 n_slices] in `dest`
    int32_t longs;             // offset (records) of its list in `longs`
    int32_t all_store;         // 1: every row of the part is stored by this kernel (no row of tiles, no mixed row: `mode` is not read)
    int32_t pad;
};
struct ColresParams {
    // Per part and K range: the slices of wave w (w, w + 16, ... of the part's length-sorted slots; per range a multiple of 4 steps wide, at least 4) back to back, in batches of 4 steps:
    // batch t of wave w, lane l at (woff[range][w] + t) * 64 + l.  Columns are relative to the range's first; a slot shorter than its slice (in that range) ends in (the range's length, 0.0f):
    // the cell behind the range's last row of B in LDS, which the kernel clears.
    const uint2* col4;         // four 16-bit columns per batch and lane
    const float4* val4;        // four values per batch and lane; nullptr: every stored value is 1.0f (unit image)
    const ColresPartDev* parts;
    const int32_t* meta;       // per part: wslice[17] (first slice of every wave in the wave-major order of bnd / dest), woff[range][17] (batches), bnd[range][slice] (the batch of
                               // its wave's stream of that range behind the slice's last one)
    const int32_t* dest;       // per part [64 n_slices] (wave-major): cell of the staging image the slot's sum goes to (row of C - r0, or an extra cell >= rows); -1: padding slot
    const ColresLong* longs;
    const uint8_t* mode;       // per row of C (padded to a multiple of 4): 0 the row is not this kernel's (a block-row of tiles), 1 store its sum, 2 add it to what the tile launches stored
    const float* B;            // column-major, ld = ldb
    int64_t ldb;
    float* C;                  // column-major, ld = ldc
    int64_t ldc;
    int32_t krange[kColresMaxRanges + 1];      // first column of every K range (multiples of 4), then cols
    int32_t n_parts, n_ranges, N, accumulate, vec_out, vec_in;
    int32_t n_cus, share, stagger_ticks;      // CUs of the device, groups the CUs of the first dispatch round start in, and the offset between the groups in 10 ns ticks (0: none) -- see the kernel
    int32_t probe;             // developer probe (SPARTA_COLRES_PROBE, wrong products): 1 skip the loads of B, 2 skip the stream of A, 4 skip the stores of C
};

// ---- column-compacted ("union-pattern") tiles of fp32 handles (k_union.hip, vbs_union.cpp; host form: sparta::UnionPlanHost) ----
struct UnionRec { int32_t c_row, info, tail_off, pad; };  // per step: first row of C of its tile; info = rows of the tile (bits 0..6) | valid list positions of this step, 0..32 (bits 8..13) | UREC_LAST
                                                         // | tail entries per row (bits 17..21); tail_off: first (column, value) pair of the tile's tail
static_assert(sizeof(UnionRec) == 16, "UnionRec must stay 16 bytes");
constexpr int32_t UREC_LAST = 1 << 16;                   // the tile's last step: add the tail, store the tile's rows of C
constexpr int UREC_TAIL_SHIFT = 17;
constexpr int kUnionPadSteps = 4;                        // records / list entries / slices behind the last step (the pipeline requests up to three steps past a worker's range)
constexpr int kUnionPairFloats = 256;    // fp32 plans: floats (1 KB) behind a step's slice of A that hold the (column, value) pairs of the tail entry the step requests
constexpr int kUnionTypes = 4;    // tile types of one handle.  fp32: type t = tiles of 16 t + 1 .. 16 (t + 1) rows (t + 1 MFMA row tiles of 16); 16-bit: types 0, 1 = tiles of <= 32 / 33..64 rows
struct UnionSide {                // one tile type
    const UnionRec* rec;          // per step, in execution order (worker after worker)
    const int32_t* ids;           // [step][32]: the rows of B (= columns of A) of the step's list positions; behind the valid ones the tile's first column (fetched: A holds zeros there)
    const void* A;                // the steps' slices as the LDS image the kernel wants.  fp32, type t (R = 16 (t + 1) rows): [step]{[rt][h][lane][4] floats, then kUnionPairFloats: the step's tail pairs [row] uint2}, lane = 16 kq + i:
                                  // A[16 rt + i][k = 4 (4 h + e) + kq] (one ds_read_b128 per lane = the row's values of four consecutive 16x16x4 MFMAs);
                                  // 16-bit, type t (32 (t + 1) rows): [step][rt][m][kg][row][8] = A[32 rt + row][k = 16 m + 8 kg + e]
    const int32_t* worker_range;  // [2 x workers]: begin, end step
    const uint2* tail;            // per tile (execution order) [entry][R rows]: (column, value bits) added in the tile's epilogue
    int32_t n_workers, c_nt;
};
struct UnionParams {              // ONE launch: workgroup b walks its range of every type (side[t].worker_range[2 b ..]), tallest type first
    UnionSide side[kUnionTypes];
    const float* B;               // ROW-major cols x n_cols, ld = ldb (a multiple of 4 elements, 16-byte aligned base)
    int64_t ldb;
    float* C;
    int64_t ldc;
    int32_t n_cols, accumulate, c_row_major, pad;
};

struct SpSegRec { int64_t p0; int32_t cnt, pad; };
struct SpLongRec { int32_t ord, seg_begin, n_seg, pad; };

struct BlockRowDesc {
    int64_t a_off, jab_off;
    int32_t nb, h, c_row, pad;
};

// SDDMM (k_sddmm.hip): one work item = one block-row, one tile of <= 32 of its rows, and up to kSdGroups groups of 32 stored columns
// (stored column q = b * w + c of the block-row, the mab order; group g = columns 32 g .. 32 g + 31)
constexpr int kSdGroups = 16;
struct SddmmItem { int32_t brow, r0, g0, ng; };
struct SddmmParams {
    const BlockRowDesc* brows;
    const int32_t* jab;
    const SddmmItem* items;
    const void* X;                  // rows x k, column-major (fp32, or the handle's 16-bit type)
    const void* Y;                  // cols x k, column-major
    float* G;                       // nztot values in the mab layout
    int64_t ldx, ldy, cols;
    int32_t k, w, accumulate, pad;
};

// the live-block set of a handle (sparta_vbs_set_live_blocks; k_live.hip writes these arrays, the live kernels of k_sddmm.hip read them): per block-row of
// d_brows the numbers of its live groups, in ascending order, at groups[goff[brow] ..], count[brow] of them (-1 behind them); keep = the snapshot, one byte
// per stored block (0 / 1), block b of block-row `brow` at keep[brows[brow].jab_off + b].  An item (brow, r0, g0, ng) takes positions g0 .. g0 + 15 of the list.
struct SddmmLive {
    const int32_t* groups;
    const int32_t* goff;
    const int32_t* count;
    const uint8_t* keep;
};
// the score form (sparta_vbs_sddmm_block_ssq): the SddmmLive of the call holds the lists of `sel`; a wave writes the fp64 sum of squares of the tile's rows of
// stored column q of block-row `brow`, tile r0 / 32, to slots[soff[brow] + (r0 / 32) * nb * w + q] -- one slot per (32-row tile, stored column) of the pattern;
// the finish kernel sums a block's ntiles x w slots (slot0 + t * tstride + c) in one fixed order
struct SddmmScore {
    double* slots;
    const int64_t* soff;
};
struct ScoreBlock { int64_t slot0, tstride; int32_t ntiles, pad; };
static_assert(sizeof(ScoreBlock) == 24, "ScoreBlock must stay 24 bytes");

// sparta_vbs_set_values (k_update.hip): where one 16-bit slice of an updatable handle comes from.  Row rr of the slice, column kk of its k range, is
// mab[off_lo + kk * h_lo + rr] for rr < rows_lo, else mab[off_hi + kk * h_hi + (rr - 32)] for 32 <= rr < 32 + rows_hi, else zero.  An ordinary tile has
// rows_lo = its rows (<= 64) and rows_hi = 0; a pair tile has rows_lo = 32 or 0 (upper block-row present or not) and rows_hi = the lower block-row's
// rows or 0; a hub slice has rows_lo = the sub-tile's height.  Offsets are relative to the handle's first stored element.
struct UpdSlice {
    int64_t off_lo, off_hi;
    int32_t h_lo, h_hi;
    int32_t rows_lo, rows_hi;
};
static_assert(sizeof(UpdSlice) == 32, "UpdSlice must stay 32 bytes");
// sparta_vbs_sgd_step (k_update.hip): the hyper-parameters of one step, as sparta_sgd_cfg carries them
struct SgdCfg { float lr, momentum, weight_decay, grad_scale; };
// the control record of sparta_grad_stats / sparta_grad_ctl_finish (k_gradctl.hip): 16 words of record + one 16-byte partial per workgroup of the largest grid
// of the reduction, which takes one workgroup per kGradCtlChunk elements (kGradCtlUnroll 16-byte loads per lane).  The steps read words 7 (coef) and 8 (skip).
constexpr int kGradCtlUnroll = 4;
constexpr int64_t kGradCtlChunk = (int64_t)kThreads * 4 * kGradCtlUnroll;
constexpr int kGradCtlMaxGrid = 1024;
constexpr size_t kGradCtlBytes = 64 + 16 * (size_t)kGradCtlMaxGrid;
constexpr int kGradCtlCoef = 7, kGradCtlSkip = 8;
// sparta_vbs_adam_step (k_update.hip): sparta_adam_cfg and the three constants the host derives from it in fp32 (omb1 = 1 - beta1, omb2 = 1 - beta2,
// dk = 1 - lr * weight_decay), and the operands of one step: W, G, M, V = nztot floats each, S = the 8-word step state
struct AdamCfg { float lr, beta1, beta2, eps, weight_decay, grad_scale, omb1, omb2, dk; int32_t decoupled; };
struct AdamArgs { float* W; const float* G; float* M; float* V; float* S; AdamCfg c; const uint32_t* R = nullptr; };   // R: the control record, or nullptr

// sparta_vbs_spmm_t (k_spmm_t.hip): Ct (+)= A^T X walks A by block column.  The index (pattern only, built at creation): per block column the list of
// its blocks, in block-row order; a work item = one panel of <= 32 stored columns of one block column x its whole list.  The image the kernel reads:
// fp32 handles the reference-layout image (block = column-major h x w: column q is h consecutive floats at off + q * h); 16-bit handles an image of
// their own, per block [ceil(h / 8)][w][8]: chunk (kc, q) = rows 8 kc .. 8 kc + 7 of stored column q at off + (kc * w + q) * 8, rows past h zero.
struct SpmmTBlock { int64_t off; int32_t h, r0; };            // element offset of the block in the image, its height, its first row of X
static_assert(sizeof(SpmmTBlock) == 16, "SpmmTBlock must stay 16 bytes");
struct SpmmTItem { int32_t jb, q0, l0, l1; };                 // block column, first stored column of the panel, blocks[l0 .. l1) (empty: the item writes zeros)
struct SpmmTSrc { int64_t src, dst; int32_t h, pad0; int64_t pad1; };   // 16-bit image: block at mab + src (column-major h x w) -> image + dst
static_assert(sizeof(SpmmTSrc) == 32, "SpmmTSrc must stay 32 bytes");
struct SpmmTParams {
    const SpmmTItem* items;
    const SpmmTBlock* blocks;
    const void* A;                  // the image (fp32 / 16-bit)
    const void* X;                  // rows x n_cols, column-major (fp32, or the handle's 16-bit type)
    float* Ct;                      // cols x n_cols, column-major
    int64_t ldx, ldo, cols;
    int32_t n_cols, w, accumulate, pad;
};
constexpr int kSpmmTSlab = 128;     // columns of X / Ct per workgroup (32 per wave)

// block pruning (k_prune.hip): one record per stored block, mab order (build_block_table, vbs_plan.cpp): its first element, the elements inside the matrix
// (the block's first n_in), all its elements
struct PruneBlock { int64_t off; int32_t n_in, n_all; };
static_assert(sizeof(PruneBlock) == 16, "PruneBlock must stay 16 bytes");
constexpr int kPruneWaves = kThreads / 64;    // blocks per workgroup: one wave each
// repattern (k_repattern.hip): one record per block of the DESTINATION handle, mab order: where its elements come from in the source layout, where they go,
// how many (n_all), and whether the block is moved (1) or new (0: zeros, nothing read)
struct MoveBlock { int64_t src_off, dst_off; int32_t n_all, moved; };
static_assert(sizeof(MoveBlock) == 24, "MoveBlock must stay 24 bytes");
// dense <-> blocks (k_dense.hip): one record per chunk of at most 64 rows of a stored block, mab order: the block's first element in the mab layout, its
// first row (from the start of the handle's range) and first column in the dense matrix, its height, the chunk's first row inside the block and its rows,
// and the block's stored columns inside the matrix.  Blocks of height 0 have no record.
struct DenseItem { int64_t off; int32_t r0, c0, h, i0, hc, valid; };
static_assert(sizeof(DenseItem) == 32, "DenseItem must stay 32 bytes");
constexpr int kDenseChunk = 64;

// the epilogue of a linear layer (k_epilogue.hip): column-major rows x n_cols operands.  A work item = a tile of kThreads rows x a run of kEpRun columns.
// Rows [head, head + 4 n4) are the body (vec_tiles tiles, a lane owns four rows: every operand is aligned there in every column), the others the edge
// (edge_tiles tiles, one element per access); ep_plan (vbs_epilogue.cpp) fills the four.  dY / Out: the types are the kernels' template arguments.
constexpr int kEpRun = 32, kEpNone = 0, kEpRelu = 1, kEpGelu = 2;
struct EpilogueParams {
    const void* dY;                 // backward only
    const float* Z;                 // forward: the input; backward: NULL allowed when act == kEpNone
    const float* bias;              // or nullptr
    void* Out;                      // Y / dZ
    float* dbias;                   // backward: nullptr = no sums
    double* part;                   // backward, n_runs > 1: n_runs x rows partial sums (the caller's scratch)
    int64_t lddy, ldz, ldo, rows, n_cols, n_runs;
    int64_t head, n4, vec_tiles, edge_tiles;
    int32_t act, pad;
};

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return sparta::fail(SPARTA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// ---- the single owners of device memory and events: nothing else in the library spells hipMalloc / hipFree / hipEventCreate / hipEventDestroy --------
// Owners free in their destructors: destroy one with its device current (DeviceGuard).  DevBuf keeps the two process-wide counters that
// sparta_debug_device_allocs reads: allocations held right now, and their bytes as asked of hipMalloc.
inline std::atomic<int64_t> g_dev_live_count{0}, g_dev_live_bytes{0};

// one allocation of T (uint8_t: a byte buffer).  Converts to T* so that launches and `if (A->d_x)` read as with a raw pointer; a reinterpreting site says .get()
template <class T>
struct DevBuf {
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; } return *this; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t bytes() const { return bytes_; }
    void reset() {
        if (p_) { (void)hipFree(p_); g_dev_live_count--; g_dev_live_bytes -= (int64_t)bytes_; }
        p_ = nullptr; bytes_ = 0;
    }
    // frees what it held first: a builder that failed half-way and is called again leaks nothing
    hipError_t alloc(size_t n_elems, size_t min_bytes = 0) {
        reset();
        const size_t b = std::max(n_elems * sizeof(T), min_bytes);
        const hipError_t e = hipMalloc((void**)&p_, b);
        if (e != hipSuccess) p_ = nullptr;
        if (p_) { bytes_ = b; g_dev_live_count++; g_dev_live_bytes += (int64_t)b; }      // (an empty allocation holds nothing)
        return e;
    }
    // n elements of src behind a fresh allocation of n + pad_elems, the padding zeroed: one size for the allocation and the copy
    hipError_t upload(const T* src, size_t n, size_t pad_elems = 0) {
        hipError_t e = alloc(n + pad_elems);
        if (e == hipSuccess && pad_elems > 0) e = hipMemset(p_ + n, 0, pad_elems * sizeof(T));
        if (e == hipSuccess && n > 0) e = hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    hipError_t upload(const std::vector<T>& v, size_t pad_elems = 0) { return upload(v.data(), v.size(), pad_elems); }
private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};

// set for the duration of a call whose stream is being captured into a graph (CaptureScope, vbs_host.hpp): what allocates, synchronises or times then
// fails with SPARTA_ERR_UNSUPPORTED instead of breaking the capture
inline thread_local bool g_capturing = false;
inline int capture_refusal(const char* what, const char* entry = "sparta_vbs_spmm") {
    return sparta::fail(SPARTA_ERR_UNSUPPORTED, std::string(entry) + ": the stream is being captured and this call still has to " + what +
                                                 " -- run it once outside the capture first");
}

// what a handle keeps for the graphs captured from its calls (sparta_vbs::retired): `captured` is set when a call under capture returns SPARTA_OK
// (CaptureScope, vbs_host.hpp); from then on a launch baked into a graph may hold the address of any scratch, so scratch that has to grow is moved here
// instead of being freed.  Freed with the handle; every buffer is smaller than its successor.
struct Retired {
    bool captured = false;
    std::vector<DevBuf<uint8_t>> bufs;
};

// grow-only scratch of a handle: ensure(need, keep) keeps what is large enough, otherwise frees and allocates `need` bytes (never under capture).  Converts
// to any pointer type, as the void* it replaces was cast at every use.
// Once the handle has been captured (keep.captured) the outgrown allocation is retired to keep.bufs, not freed: a captured graph may replay on it.
struct DevScratch {
    size_t bytes() const { return buf_.bytes(); }
    void* get() const { return buf_.get(); }
    template <class U> operator U*() const { return (U*)buf_.get(); }
    explicit operator bool() const { return buf_.get() != nullptr; }
    int ensure(size_t need, Retired& keep) {
        if (buf_.bytes() >= need) return SPARTA_OK;
        if (g_capturing) return capture_refusal("allocate scratch memory");
        if (keep.captured && buf_.get()) {
            keep.bufs.emplace_back();                            // (first: if the list cannot grow, nothing has moved)
            keep.bufs.back() = std::move(buf_);
        }
        HIP_TRY(buf_.alloc(need));
        return SPARTA_OK;
    }
private:
    DevBuf<uint8_t> buf_;
};

struct DevEvent {
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    ~DevEvent() { if (ev_) (void)hipEventDestroy(ev_); }
    hipError_t create() { return ev_ ? hipSuccess : hipEventCreate(&ev_); }
    operator hipEvent_t() const { return ev_; }
private:
    hipEvent_t ev_ = nullptr;
};

}  // namespace sparta_dev

struct sparta_vbs {
    int device = 0, dtype = SPARTA_F32;
    int64_t rows = 0, cols = 0, block_rows = 0, w = 0, nblocks = 0, nztot = 0;
    sparta_dev::DevBuf<float> d_A;                    // fp32: the reference's mab; 16-bit handles: packed slices (see sparta_vbs_create)
    int kp16 = 0;                            // 16-bit handles: k depth of a step (32 or 64)
    sparta_dev::DevBuf<int32_t> d_jab;
    sparta_dev::DevBuf<sparta_dev::TileDesc> d_tiles[4];   // classes 16, 32, 64, 128
    int64_t n_tiles[4] = {0, 0, 0, 0};       // launch entries (real tiles + padding)
    int64_t n_real_tiles[4] = {0, 0, 0, 0};
    sparta_dev::DevBuf<sparta_dev::BlockRowDesc> d_brows;
    int64_t n_brows = 0;
    int64_t exec_area = 0;
    int64_t a_bytes = 0;
    sparta_dev::DevEvent ev0, ev1;
    sparta_dev::DevEvent cev[4][2];
    bool class_timing = false;
    bool class_ran[4] = {false, false, false, false};
    // stream plan (w % 32 == 0): see vbs_spmm_f32_stream_kernel
    sparta_dev::DevBuf<sparta_dev::StepRec> d_steps[2];      // per tile type: [0] <= 32 rows, [1] 33..64 rows
    std::vector<sparta_dev::StepRec> h_steps[2];               // host copies (padded), source of the gathered-B variants
    // step lists for sparta_vbs_spmm_gathered: one set per slab height the handle has been called with, kept until destroy and never rewritten (a graph
    // captured at one height replays on that height's lists whatever heights are called later); g_cur = the set of the last call's height, -1: none yet
    struct GatheredSteps {
        int64_t shard_rows = 0;
        sparta_dev::DevBuf<sparta_dev::StepRec> steps[2];     // per tile type, as d_steps
        sparta_dev::DevBuf<sparta_dev::HubStep> hub;          // as d_hub_steps
    };
    std::vector<GatheredSteps> gathered;
    int g_cur = -1;
    sparta_dev::Retired retired;                              // outgrown scratch a captured graph may still replay on (DevScratch::ensure)
    sparta_dev::DevBuf<int32_t> d_wrange[2];
    sparta_dev::DevBuf<sparta_dev::FixRec> d_fix;
    std::vector<std::pair<int64_t, int64_t>> zero_ranges;   // long runs of rows without blocks (local C rows), see vbs_zero_rows_kernel
    sparta_dev::DevBuf<int32_t> d_fix_slots;
    int64_t n_steps[2] = {0, 0};
    int32_t n_workers = 0, n_fix = 0, n_split = 0, n_slots = 0;
    int32_t max_tile_slots = 0;            // most partial images of one split tile
    sparta_dev::DevBuf<int32_t> d_big_fix;          // fix records with more than 2 * kFixGroup images (group stage)
    int32_t n_big_fix = 0;
    sparta_dev::DevScratch d_ws;
    int64_t n_plan_tiles[2] = {0, 0};             // see StreamPlanHost
    bool tiles_row_aligned[2] = {true, true};
    bool wide16 = false;                      // the 16-bit one-tile plan holds two sub-worker ranges per workgroup (vbs_spmm_h16_direct_kernel, WC = 64)
    sparta_dev::DevBuf<float> d_a_frag;                    // A of the one-tile plan in fragment order (k_f32_direct.hip) or nullptr
    sparta_dev::DevBuf<float> d_a_pack;                    // packed handles (k_f32_packed.hip): A per PACKED step, instead of d_a_frag
    sparta_dev::DevBuf<sparta_dev::StepRec> d_psteps;      // ... the packed steps, their worker ranges, and where every block of d_steps[0] sits in d_a_pack
    sparta_dev::DevBuf<int32_t> d_pwrange;
    sparta_dev::DevBuf<sparta_dev::PackLoc> d_pack_loc;
    int64_t n_psteps = 0, pack_slots = 0;
    bool legacy_dropped = false;                  // fp32: the reference-layout image d_A was freed once the fragment image had won (rebuilt on demand, then kept)
    // hub plan (16-bit handles of 64-wide blocks; vbs_plan.cpp, k_hub16.hip)
    sparta_dev::DevBuf<sparta_dev::HubStep> d_hub_steps;
    std::vector<sparta_dev::HubStep> h_hub_steps; // host copy (padded), source of the gathered variant
    sparta_dev::DevBuf<sparta_dev::HubTile> d_hub_tiles;
    sparta_dev::DevBuf<int32_t> d_hub_wrange;
    sparta_dev::DevBuf<uint16_t> d_hub_A;
    int hub_g = 0, hub_workers = 0;
    int64_t n_hub_steps = 0, hub_area = 0, hub_union_area = 0, n_hub_tiles = 0, n_hub_groups = 0, hub_chunks = 0, hub_segments = 0;
    bool has_tail = false;                 // cols % w != 0: the stream path needs B_tail
    sparta_dev::DevScratch d_btail;
    int last_path = 0;                     // 1: stream kernel, 2: per-class branch-free kernels, 3: per-class generic kernels
    std::vector<std::pair<int64_t, int>> tuned;   // (n_cols/layout key) -> measured best path
    float tune_ms[2] = {0.0f, 0.0f};
    sparta_dev::DevScratch d_tune;
    sparta_dev::DevScratch d_B16;                 // 16-bit handles, host-pointer calls: B converted on the device
    sparta_dev::DevScratch d_Bt;                  // 16-bit handles, n_cols % 128 != 0: the last n_cols % 128 columns of B, zero-padded to a 128-column slab
    sparta_dev::DevScratch d_Ct;                  // ... and the 128-column slab of C they produce (column-major, ld = rows), merged into C afterwards
    sparta_dev::DevBuf<long long> d_clk;           // clock probe: [4 launches][4] = {s_memtime, s_memrealtime} at entry, at exit
    sparta_dev::DevEvent tev0, tev1;
    // sparse-row path (fp32 handles): the block-rows taken out of the MFMA plans, as rows of (column, value)
    int64_t n_sp_rows = 0, n_sp_short = 0, n_sp_long = 0, sp_nnz = 0;
    bool ext_sparse = false;               // created from CSR: the sparse rows have no dense image (no exact-order kernel for them)
    sparta_dev::DevBuf<int64_t> d_sp_rowptr;
    sparta_dev::DevBuf<int32_t> d_sp_col;
    sparta_dev::DevBuf<float> d_sp_val;
    sparta_dev::DevBuf<int32_t> d_sp_crow;
    sparta_dev::DevBuf<int32_t> d_sp_list;          // the short rows (one wave each)
    sparta_dev::DevBuf<sparta_dev::SpSegRec> d_sp_segs;             // SpSegRec[n_sp_segs]: segments of the long rows
    sparta_dev::DevBuf<sparta_dev::SpLongRec> d_sp_long;             // SpLongRec[n_sp_long]
    int64_t n_sp_segs = 0;
    sparta_dev::DevBuf<int32_t> d_sp_stream_begin;  // XCD-affine order of the segments: eight streams, [9] offsets into d_sp_segs (nullptr: one list, window-major)
    int64_t sp_max_stream = 0;
    sparta_dev::DevScratch d_sp_part;             // partial rows of the segments
    // resident-column product (k_colres.hip): fp32 handles whose rows are ALL sparse rows and whose columns of B fit LDS
    sparta_dev::DevBuf<uint16_t> d_cr_col;               // 16-bit columns
    sparta_dev::DevBuf<float> d_cr_val;               // values (nullptr: unit image)
    sparta_dev::DevBuf<int32_t> d_cr_meta;          // woff[17], wslice[17], bnd[n_slices]
    sparta_dev::DevBuf<int32_t> d_cr_dest;
    sparta_dev::DevBuf<sparta_dev::ColresLong> d_cr_longs;
    int32_t cr_slices = 0, cr_long = 0, cr_plane = 0, cr_lmax = 0;       // slices of the part with most; rows cut into chunks; cells of the largest staging image / range of B; longest slot
    int32_t cr_parts = 0, cr_ranges = 0, cr_span = 0;
    int32_t cr_krange[sparta_dev::kColresMaxRanges + 1] = {0, 0, 0, 0, 0};
    sparta_dev::DevBuf<sparta_dev::ColresPartDev> d_cr_parts;
    sparta_dev::DevBuf<uint8_t> d_cr_mode;
    bool cr_unit = false;                  // every value 1.0f: no value array
    // ... and the same matrix once more in FOUR parts of the rows of C, for products of few column sets (N <= 128 with two columns per workgroup): 4 x the workgroups, each with a
    // quarter of the stream of A -- with fewer workgroups than CUs one workgroup's stream IS the product's time
    struct ColresSmall {
        sparta_dev::DevBuf<uint16_t> col; sparta_dev::DevBuf<float> val; sparta_dev::DevBuf<int32_t> meta, dest; sparta_dev::DevBuf<sparta_dev::ColresLong> longs; sparta_dev::DevBuf<sparta_dev::ColresPartDev> parts;
        int32_t slices = 0, plane = 0, n_parts = 0;
    } cr_small;
    bool last_colres_small = false;        // the last product on this path used the four-part image
    int64_t cr_entries = 0;                // stored entries, padding included
    int last_colres_nc = 0;                // columns per workgroup of the last product on this path (0: the product took another path)
    // column-compacted tiles (fp32 handles made from a CSR: vbs_build.cpp mode 3): per tile type [0] <= 32 rows, [1] 33..64 rows
    sparta_dev::DevBuf<sparta_dev::UnionRec> d_u_rec[sparta_dev::kUnionTypes];
    sparta_dev::DevBuf<int32_t> d_u_ids[sparta_dev::kUnionTypes];
    sparta_dev::DevBuf<uint8_t> d_u_a[sparta_dev::kUnionTypes];
    sparta_dev::DevBuf<int32_t> d_u_wrange[sparta_dev::kUnionTypes];
    sparta_dev::DevBuf<uint32_t> d_u_tail[sparta_dev::kUnionTypes];
    int32_t u_workers[sparta_dev::kUnionTypes] = {0, 0, 0, 0};
    int64_t u_steps[sparta_dev::kUnionTypes] = {0, 0, 0, 0}, u_tiles[sparta_dev::kUnionTypes] = {0, 0, 0, 0};   // per tile type of the DEVICE plan
    int64_t u_tiles_h[2] = {0, 0}, u_steps_h[2] = {0, 0}, u_steps_total = 0;   // tiles / steps of tiles of <= 32 / 33..64 rows; all steps
    int64_t u_area = 0, u_cols = 0, u_nnz = 0;      // stored elements (rows x list entries), list entries, nonzeros held (lists + tails)
    int64_t u_tail_nnz = 0, u_rows = 0;             // nonzeros in the tiles' tails; rows of C the tiles own
    int64_t u_exec_area = 0;                        // elements the kernel multiplies: steps x 32 x rows of the tile's type
    const void* brm_ready = nullptr;       // the row-major B of the product in flight (set by the first launch that needs it, cleared when the product returns)
    int64_t brm_ld = 0;
    sparta_dev::DevScratch d_Brm;                 // row-major copy of a column-major / gathered B
    const void* prepared_brm = nullptr;    // set for the duration of a sparta_vbs_spmm_prepared call: the caller's row-major copy, made once
    int64_t prepared_ld = 0;               // ... and its row stride (the n_cols it was prepared for: a 16-bit call with n_cols % 128 != 0 is cut into sub-calls)
    sparta_dev::DevScratch d_B;
    sparta_dev::DevScratch d_C;
    // SDDMM (sparta_vbs_sddmm): the work list, built at the first call; host-pointer calls stage X, Y, G (and 16-bit X, Y) in scratch
    sparta_dev::DevBuf<sparta_dev::SddmmItem> d_sd_items;
    int64_t n_sd_items = -1;               // -1: not built yet
    sparta_dev::DevScratch d_sd_ws;
    sparta_dev::DevScratch d_sd_h16;
    // sparta_vbs_set_values (SPARTA_CREATE_UPDATABLE handles only): the source of every 16-bit slice, in image order; host-pointer calls stage mab in scratch
    int32_t create_flags = 0;
    sparta_dev::DevBuf<sparta_dev::UpdSlice> d_upd_map[2];   // per tile type: one record per step (= slice) of d_A
    int64_t upd_base[2] = {0, 0};                              // element offset of the type's first slice in d_A
    sparta_dev::DevBuf<sparta_dev::UpdSlice> d_upd_hub;                 // one record per 64 x 64 slice of d_hub_A
    int64_t n_upd_hub = 0;
    sparta_dev::DevScratch d_upd_ws;
    // sparta_vbs_sgd_step: stored elements the slices of each stream image hold (set at creation from the plan: an image that holds nztot of them, the only
    // non-empty one, holds each exactly once and its kernel may own the arithmetic); what the last step of either optimizer did (sparta_vbs_step_info)
    int64_t upd_cover[2] = {0, 0};
    int32_t step_last_fused = -1, step_last_launches = 0;
    // sparta_vbs_spmm_t (SPARTA_CREATE_TRANSPOSE handles only): the block-column index, the 16-bit image, the sources of its blocks; host-pointer calls stage X, Ct
    sparta_dev::DevBuf<sparta_dev::SpmmTItem> d_t_items;
    sparta_dev::DevBuf<sparta_dev::SpmmTBlock> d_t_blocks;
    int64_t n_t_items = 0, n_t_blocks = 0;
    sparta_dev::DevBuf<uint16_t> d_t_A;                                 // 16-bit handles: [ceil(h / 8)][w][8] per block, blocks in mab order
    sparta_dev::DevBuf<sparta_dev::SpmmTSrc> d_t_src;                   // 16-bit handles with both flags: one record per block (set_values)
    int64_t n_t_src = 0;
    sparta_dev::DevScratch d_t_ws;
    sparta_dev::DevScratch d_t_h16;
    // block pruning (sparta_vbs_block_ssq / sparta_vbs_mask_blocks; handles made from VBS arrays only): the block-rows' heights and block counts, kept from
    // creation, and the block table, built from them and the handle's jab and uploaded at the first call
    bool from_vbs_arrays = false;
    std::vector<int64_t> h_row_part, h_nzcount;                // [block_rows + 1] (from 0), [block_rows]
    sparta_dev::DevBuf<sparta_dev::PruneBlock> d_prune;
    int64_t n_prune = -1;                                      // -1: not built yet
    // repattern (sparta_vbs_move_blocks with this handle as the destination): the records of the last call, grown when needed
    sparta_dev::DevScratch d_repat;
    // dense <-> blocks (sparta_vbs_gather_dense / sparta_vbs_scatter_dense): the chunk records, built from the same rows as the block table and uploaded at
    // the first call; whether a block-row stores a block column twice (scatter is refused then: two blocks would write the same elements of D)
    sparta_dev::DevBuf<sparta_dev::DenseItem> d_dense;
    int64_t n_dense = -1;                                      // -1: not built yet
    bool dense_dup = false;
    // the live-block set (sparta_vbs_set_live_blocks): whether one is installed is host state; the helper arrays (pattern only) are built at the first call,
    // the snapshot and the compacted lists are written by the launches of every call (k_live.hip)
    bool live_on = false, live_built = false;
    sparta_dev::DevBuf<uint8_t> d_live_keep;                            // [nblocks] the snapshot (0 / 1)
    sparta_dev::DevBuf<int32_t> d_live_goff;                            // [n_brows] first position of the block-row's slice of d_live_groups
    sparta_dev::DevBuf<int32_t> d_live_groups;                          // [live_n_groups]
    sparta_dev::DevBuf<int32_t> d_live_gcount;                          // [n_brows]
    int64_t live_n_groups = 0;
    sparta_dev::DevBuf<int32_t> d_live_tmap;                            // [live_n_tlist] list position of d_t_blocks -> block number
    sparta_dev::DevBuf<int32_t> d_live_tids;                            // [live_n_tlist] the live block numbers of every block column, compacted (-1 behind them)
    sparta_dev::DevBuf<int32_t> d_live_tcount;                          // [block columns]
    sparta_dev::DevBuf<sparta_dev::SpmmTBlock> d_live_t_blocks;         // d_t_blocks, every block column's live records first
    sparta_dev::DevBuf<sparta_dev::SpmmTItem> d_live_t_items;           // d_t_items with l1 = l0 + live count
    int64_t live_n_tlist = 0, live_block_cols = 0;
    // live steps (sparta_vbs_set_live_steps): the switch is host state and acts only while a live set is installed.  Handles with a fused image hold one
    // word per step (fp32) / two per slice (16-bit) for its kernel: the map word -> block number is pattern only (built at the first enabling call), the words
    // are written from the snapshot by one launch of k_live.hip.  The two-pass form needs nothing of its own: it walks d_prune with d_live_keep.
    bool live_steps = false, live_steps_built = false;
    bool live_words_built = false;                             // the word map and the words exist (live steps or live forward asked for them)
    sparta_dev::DevBuf<int32_t> d_live_wmap;                            // [live_n_words]
    sparta_dev::DevBuf<uint32_t> d_live_words;                          // [live_n_words]
    int64_t live_n_words = 0;
    int32_t step_last_live = 0;                                // the last step skipped dead blocks (sparta_vbs_step_info word 2)
    // live forward (sparta_vbs_set_live_forward): the switch is host state and acts only while a live set is installed.  Handles that have the word map
    // (16-bit, one stream image, no hub plan) hold a second record array and a second range array for that image; k_live.hip rewrites them from the live
    // words behind every set_live_blocks, and the live kernels of k_h16_live.hip walk them.  The plain arrays are never written.
    bool live_fwd = false, live_fwd_built = false;
    int live_fwd_ty = -1;                                      // the stream image that has the live form, -1: none (the plain kernels run under the switch)
    sparta_dev::DevBuf<sparta_dev::StepRec> d_fwd_steps;                // [n_steps[ty] + padding] d_steps[ty], every range's kept steps first
    sparta_dev::DevBuf<int32_t> d_fwd_wrange;                           // the live ranges, as d_wrange[ty]
    sparta_dev::DevBuf<int32_t> d_fwd_seg_last;                         // [n_steps[ty]] last record of every step's segment (pattern only)
    int64_t fwd_n_ranges = 0, fwd_n_alloc = 0;
    int32_t fwd_last_form[2] = {0, 0};                         // per stream image: the form the last 16-bit product ran (0 none yet, 1 plain, 2 live, 3 a8, 4 a8 live)
    // the fp8 weight image (sparta_vbs_set_forward_a8): the switch is host state.  The first enabling call allocates the e4m3 image of the one stream image (the
    // slices of d_A in the same order, one byte per element, the same padding behind them) and a private copy of its step records whose last word holds the
    // biased exponents of the slice's two groups.  vbs_a8quant_kernel rewrites both behind every write of values while the switch is on.
    bool a8_on = false, a8_built = false, a8_valid = false;
    int a8_ty = -1;                                            // the stream image that has the a8 form
    sparta_dev::DevBuf<uint8_t> d_a8;                                   // [a8_bytes]
    sparta_dev::DevBuf<sparta_dev::StepRec> d_a8_steps;                 // [n_steps[a8_ty] + padding]
    int64_t a8_bytes = 0, a8_n_groups = 0, a8_launches = 0;
    // the fp8 image with a live-block set (sparta_vbs_set_a8_live): host state; acts while a8 is on and valid and a live set is installed.  The product then walks
    // the compacted records of live forward (d_fwd_steps, d_fwd_wrange: live_fwd is off by the refusals, so they have no other reader) on d_a8, and
    // vbs_q8lv_scales_kernel keeps the exponent words in their last words, behind every compaction and every quantise launch.
    bool a8_live = false;
    int64_t a8_live_launches = 0;
    // block scores of the SDDMM (sparta_vbs_sddmm_block_ssq): a second snapshot / group list / count, written from `sel` by every call (goff is d_live_goff:
    // pattern only), the all-ones selection that stands in for sel == NULL, and the pattern-only slot offsets, finish records and the fp64 slots themselves
    bool score_built = false;
    sparta_dev::DevBuf<uint8_t> d_score_keep;                           // [nblocks] the snapshot of sel
    sparta_dev::DevBuf<uint8_t> d_score_ones;                           // [nblocks] 1
    sparta_dev::DevBuf<int32_t> d_score_groups;                         // [live_n_groups]
    sparta_dev::DevBuf<int32_t> d_score_gcount;                         // [n_brows]
    sparta_dev::DevBuf<int64_t> d_score_soff;                           // [n_brows] first slot of the block-row
    sparta_dev::DevBuf<sparta_dev::ScoreBlock> d_score_blocks;          // [nblocks]
    sparta_dev::DevBuf<double> d_score_slots;                           // [sum over block-rows of ceil(h / 32) * nb * w]
};

namespace sparta_dev {

// ---- launch functions exported by the kernel translation units ------------------------------------------------------
// k_f32_class.hip
void launch_f32_class(int cls, bool b_row_major, bool generic, const SpmmParams& p, hipStream_t st);
void launch_f32_exact(unsigned n_brows, hipStream_t st, const BlockRowDesc* rows, const int32_t* jab, const float* A, const float* B, float* C,
                      int64_t ldb, int64_t ldc, int64_t cols, int N, int w, int b_row_major, int c_row_major, int accumulate, int64_t shard_rows,
                      int64_t shard_stride);
// k_f32_stream.hip
void launch_f32_stream(bool mi2, bool b_row_major, bool gathered, dim3 grid, hipStream_t st, const StreamParams& sp);
void launch_f32_direct(bool c_stage, dim3 grid, hipStream_t st, const StreamParams& sp);
void launch_f32_legacy_from_frag(hipStream_t st, const StepRec* steps, int64_t n_steps, const float* a_frag, float* A);
// k_f32_packed.hip
void launch_f32_packed(bool c_stage, dim3 grid, hipStream_t st, const StreamParams& sp);
void launch_f32_legacy_from_pack(hipStream_t st, const StepRec* steps, const PackLoc* loc, int64_t n_steps, const float* a_pack, float* A);
void launch_fixup_group(dim3 grid, hipStream_t st, const FixRec* fix, const int32_t* big, const int32_t* fix_slots, float* ws_all, int64_t ws_slab_stride);
void launch_fixup(dim3 grid, hipStream_t st, const FixRec* fix, const int32_t* fix_slots, const float* ws_all, int64_t ws_slab_stride, float* C, int64_t ldc,
                  int c_row_major, int accumulate);
void launch_tail_copy(hipStream_t st, const float* B, int64_t ldb, int b_row_major, int64_t row0, int64_t cols, int w, int N, float* B_tail);
void launch_zero_rows(dim3 grid, hipStream_t st, float* C, int64_t ldc, int c_row_major, int64_t row0, int64_t nrows, int N);
// k_h16.hip
void launch_h16_stream(int kp, bool mi2, bool bf16, bool gathered, bool c_stage, bool wide, dim3 grid, hipStream_t st, const StreamParams& sp);
void launch_h16_slab256(bool bf16, dim3 grid, hipStream_t st, const StreamParams& sp);   // one-tile plans of 32-wide blocks, 256-column slabs (grid.y = N / 256), no split tile
bool h16_uses_direct_kernel(int kp, bool mi2);
void launch_h16_quad(int kp, bool bf16, bool gathered, dim3 grid, hipStream_t st, const StreamParams& sp);
// k_hub16.hip
void launch_h16_hub(int variant, bool bf16, bool gathered, hipStream_t st, const HubParams& p);
int hub_variant_kp(int variant);
int hub_variant_g(int variant);
void launch_tail_copy_h16(hipStream_t st, const uint16_t* B, int64_t ldb, int64_t row0, int64_t cols, int w, int N, uint16_t* B_tail);
void launch_convert_h16(bool bf16, hipStream_t st, const float* src, int64_t ld_in, int64_t rows, int64_t n_cols, uint16_t* dst, int64_t ld_out);
// C[:, col0 + j] (+)= Ct[:, j] for j < n_t: the column tail of a 16-bit product (Ct column-major, ld = rows)
void launch_col_tail_merge(hipStream_t st, const float* Ct, int64_t rows, float* C, int64_t ldc, int c_row_major, int col0, int n_t, int accumulate);
// k_sparse.hip
void launch_sparse_kernels(int vec, int bk, const SparseParams& q, unsigned gy, hipStream_t st, const int32_t* list, int64_t n_short, const SpSegRec* segs,
                           int64_t n_segs, const SpLongRec* longs, int64_t n_long, float* part, const int32_t* stream_begin = nullptr, int64_t max_stream = 0);
void launch_b_to_row_major(bool is16, unsigned grid, hipStream_t st, const void* B, int64_t ldb, int64_t shard_rows, int64_t shard_stride, int64_t rows, int N,
                           void* out, int64_t ld_out);
// k_union.hip
void launch_union_f32(unsigned n_slabs, hipStream_t st, const UnionParams& p);
void launch_union_h16(bool bf16, unsigned n_slabs, hipStream_t st, const UnionParams& p);   // 16-bit handles: p.B = the row-major 16-bit B, side.A = 16-bit slices
// k_sddmm.hip: one workgroup per work item (n_items <= 2^31 - 1); dtype = SPARTA_F32 / F16 / BF16
void launch_sddmm(int dtype, unsigned n_items, hipStream_t st, const SddmmParams& p);
// ... with a live set: an item's groups come from lv's compacted list, stored columns of dead blocks are not loaded (accumulate = 0: stored as +0.0f; 1: skipped);
// the groups that are not on the list are not written: under accumulate = 0 the caller zeroes the dead blocks first (launch_mask_blocks with the snapshot)
void launch_sddmm_live(int dtype, unsigned n_items, hipStream_t st, const SddmmParams& p, const SddmmLive& lv);
// ... the score form: the live form on the lists of `sel` (lv), p.G unused; instead of storing, every wave writes its slots of sc.  Then one wave per block:
// ssq[b] = the sum of the block's slots, +0.0 where snap[b] == 0
void launch_sddmm_score(int dtype, unsigned n_items, hipStream_t st, const SddmmParams& p, const SddmmLive& lv, const SddmmScore& sc);
void launch_sddmm_score_finish(hipStream_t st, const ScoreBlock* blocks, int64_t n_blocks, int w, const uint8_t* snap, const double* slots, double* ssq);
// k_update.hip (sparta_vbs_set_values): new values, nztot floats in the mab layout, into the images of an updatable handle
void launch_update_copy(hipStream_t st, const float* mab, int64_t n, float* A);        // the reference-layout image (fp32 handles)
// the fragment image of the fp32 one-tile plan, k-compaction redone per step (position table, fragments, STEP_KPAIRS of steps[q].mt_flags);
// A_out != nullptr: the steps cover every stored element, the reference-layout image is written from the same read
void launch_update_f32_frag(hipStream_t st, StepRec* steps, int64_t n_steps, const float* mab, float* a_frag, float* A_out);
// 16-bit slices of tms rows x kp columns ([k / 8][row][8]; hub: the swizzled 64 x 64 image of k_hub16.hip), rounded as to_h16 rounds
void launch_update_h16(bool bf16, bool hub, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const float* mab, uint16_t* dst);
// the 16-bit image of the transposed product, one workgroup pass per block (rounded as to_h16 rounds)
void launch_update_h16_t(bool bf16, hipStream_t st, const SpmmTSrc* src, int64_t n_blocks, int w, const float* mab, uint16_t* dst);
// k_update.hip (sparta_vbs_sgd_step): W, G, M = nztot floats each in the mab layout (M is not touched when cfg.momentum == 0)
// R (all three launches, and AdamArgs::R): the control record whose coef multiplies g and whose skip flag leaves W (and M) as they are, or nullptr
void launch_sgd_step(hipStream_t st, int64_t n, float* W, const float* G, float* M, const SgdCfg& cfg, const uint32_t* R);     // the arithmetic alone; the set_values launches follow it
// the arithmetic inside the image kernel whose image holds every stored element exactly once: launch_update_f32_frag / launch_update_h16 (stream slices) with
// the new weight computed in registers, stored to W (and M) and handed on to the image
void launch_sgd_f32_frag(hipStream_t st, StepRec* steps, int64_t n_steps, float* W, const float* G, float* M, const SgdCfg& cfg, const uint32_t* R, float* a_frag, float* A_out);
void launch_sgd_h16(bool bf16, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, float* W, const float* G, float* M, const SgdCfg& cfg, const uint32_t* R, uint16_t* dst);
// k_update.hip (sparta_vbs_adam_step): the tick advances a.S once per step; the others are the Adam forms of the three launches above and read what it wrote
void launch_adam_tick(hipStream_t st, const AdamArgs& a);
void launch_adam_step(hipStream_t st, int64_t n, const AdamArgs& a);
void launch_adam_f32_frag(hipStream_t st, StepRec* steps, int64_t n_steps, const AdamArgs& a, float* a_frag, float* A_out);
void launch_adam_h16(bool bf16, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const AdamArgs& a, uint16_t* dst);
// the live forms (sparta_vbs_set_live_steps with a live set installed).  Image kernels: `words` = the live words of launch_live_step_words, one per step / two per
// slice; a step or chunk of a dead block is neither loaded nor stored and its part of the image is +0.0.  Two-pass: the block table and the snapshot, one wave
// per block, dead blocks untouched; the set_values launches follow as behind launch_sgd_step / launch_adam_step
void launch_sgd_blocks_live(hipStream_t st, const PruneBlock* blocks, int64_t n_blocks, const uint8_t* keep, float* W, const float* G, float* M, const SgdCfg& cfg,
                            const uint32_t* R);
void launch_sgd_f32_frag_live(hipStream_t st, StepRec* steps, int64_t n_steps, float* W, const float* G, float* M, const SgdCfg& cfg, const uint32_t* R, float* a_frag,
                              float* A_out, const uint32_t* words);
void launch_sgd_h16_live(bool bf16, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, float* W, const float* G, float* M, const SgdCfg& cfg,
                         const uint32_t* R, uint16_t* dst, const uint32_t* words);
void launch_adam_blocks_live(hipStream_t st, const PruneBlock* blocks, int64_t n_blocks, const uint8_t* keep, const AdamArgs& a);
void launch_adam_f32_frag_live(hipStream_t st, StepRec* steps, int64_t n_steps, const AdamArgs& a, float* a_frag, float* A_out, const uint32_t* words);
void launch_adam_h16_live(bool bf16, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const AdamArgs& a, uint16_t* dst, const uint32_t* words);
// k_spmm_t.hip: grid = n_items x slabs of kSpmmTSlab columns; dtype = SPARTA_F32 / F16 / BF16
void launch_spmm_t(int dtype, unsigned n_items, hipStream_t st, const SpmmTParams& p);
// k_colres.hip
int launch_colres(int nc, const ColresParams& p, size_t lds_bytes, hipStream_t st);     // nc = 1..4 columns per workgroup; 0 or a hipError_t
int colres_max_slices(int nc);                                                          // slices the nc-column kernel holds sums for
void launch_pack_blocks(dim3 grid, hipStream_t st, const void* src, const int32_t* ids, void* dst, int64_t block_vec);
// k_gradctl.hip: G (n floats, any 4-byte boundary) folded into words 0..2 of the control record R (8-byte aligned, kGradCtlBytes); the finish kernel
void launch_grad_stats(hipStream_t st, const float* G, int64_t n, void* R, bool accumulate);
void launch_grad_ctl_finish(hipStream_t st, void* R, float max_norm, float growth_factor, float backoff_factor, int32_t growth_interval);
// k_prune.hip: one wave per block of the table.  ssq[b] = the fp64 sum of the exact squares of the block's first n_in elements of W; the blocks with
// keep[b] == 0 stored as +0.0f (all n_all elements) in each non-NULL T[0..3]
void launch_block_ssq(hipStream_t st, const PruneBlock* blocks, int64_t n_blocks, const float* W, double* ssq);
void launch_mask_blocks(hipStream_t st, const PruneBlock* blocks, int64_t n_blocks, const uint8_t* keep, float* T0, float* T1, float* T2, float* T3);
// k_repattern.hip: one wave per record; per non-NULL pair (S[q], D[q]) the block copied bit for bit from the source layout or stored as +0.0f
void launch_move_blocks(hipStream_t st, const MoveBlock* blocks, int64_t n_blocks, const float* const* S, float* const* D);
// k_dense.hip: one wave per record (gather: T written from D, the stored positions past cols as +0.0f; scatter: D written from T); the rows x cols region
// of D stored as +0 (dense_fill_segs: its workgroups per run); one wave per block of the (row_part, w) grid for the fp64 sums of squares
void launch_dense_gather(hipStream_t st, const DenseItem* items, int64_t n_items, const void* D, int64_t ldd, int row_major, int dtype, int w, float* T);
void launch_dense_scatter(hipStream_t st, const DenseItem* items, int64_t n_items, const float* T, void* D, int64_t ldd, int row_major, int dtype);
int64_t dense_fill_segs(int64_t run_bytes);
void launch_dense_fill(hipStream_t st, void* D, int64_t ldd, int row_major, int dtype, int64_t rows, int64_t cols);
void launch_dense_block_ssq(hipStream_t st, const void* D, int64_t ldd, int row_major, int dtype, int64_t rows, int64_t cols, int64_t block_rows, int64_t w,
                            const int64_t* row_part, double* ssq_out);
// k_epilogue.hip: Y = act(Z + bias); dZ = dY * act'(Z + bias), and with p.dbias the fixed-order fp64 row sums (a second launch folds the runs when n_runs != 1)
void launch_epilogue_fwd(hipStream_t st, int y_dtype, const EpilogueParams& p);
void launch_epilogue_bwd(hipStream_t st, int dy_dtype, int dz_dtype, const EpilogueParams& p);
// k_live.hip: the snapshot of keep and the compacted lists, one wave per block-row / per block column, stable, no atomics, no LDS
void launch_live_sddmm(hipStream_t st, const BlockRowDesc* brows, int64_t n_brows, int w, const uint8_t* keep, int64_t n_blocks, uint8_t* snap, const int32_t* goff,
                       int32_t* groups, int32_t* count);
void launch_live_spmm_t(hipStream_t st, const SpmmTItem* items, const SpmmTBlock* blocks, const int32_t* tmap, int64_t block_cols, int panels, const uint8_t* keep,
                        SpmmTItem* live_items, SpmmTBlock* live_blocks, int32_t* live_ids, int32_t* live_count);
// ... and the live words of the steps' image kernels: words[i] = all ones if block wmap[i] is live in the snapshot, else 0 (wmap[i] < 0: 0)
void launch_live_step_words(hipStream_t st, const int32_t* wmap, int64_t n_words, const uint8_t* snap, uint32_t* words);
// ... and live forward: the records of one stream image compacted per range from the live words (two per step), the rule of live_forward_compact_host
void launch_live_forward_compact(hipStream_t st, const StepRec* steps, const int32_t* seg_last, const int32_t* ranges, int64_t n_ranges, const uint32_t* words, bool pair,
                                 StepRec* out, int32_t* ranges_out);
// k_h16_live.hip: the live form of the no-barrier 16-bit kernel on those records (B not gathered, loads three steps ahead); k_h16.hip says whether the launch
// that launch_h16_stream would make has a live sibling
void launch_h16_live_stream(int kp, bool mi2, bool bf16, bool c_stage, bool wide, dim3 grid, hipStream_t st, const StreamParams& sp);
void launch_h16_live_slab256(bool bf16, dim3 grid, hipStream_t st, const StreamParams& sp);
void launch_h16_live_quad(int kp, bool bf16, dim3 grid, hipStream_t st, const StreamParams& sp);
bool h16_live_form_available(int kp, bool mi2, bool c_stage, bool wide);
// k_h16_a8.hip: the a8 form of the same launches on the handle's private records (the 128-column kernels only: a launch that would take the 256-column slab or the
// four-accumulator form takes the 128-column sibling of its plan), and the kernel that writes the e4m3 image and the exponents from nztot floats in the mab layout
void launch_h16_a8_stream(int kp, bool mi2, bool bf16, bool c_stage, bool wide, dim3 grid, hipStream_t st, const StreamParams& sp);
void launch_a8_quantize(int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const float* mab, uint8_t* dst, StepRec* recs);
// k_h16_a8_live.hip: the a8 form on the compacted records of live forward (the launches of launch_h16_a8_stream), and the kernel that copies the exponent word of
// every slice (a8_recs[s].pad) into the compacted record whose a_off = base + s * slice names it
void launch_h16_a8_live_stream(int kp, bool mi2, bool bf16, bool c_stage, bool wide, dim3 grid, hipStream_t st, const StreamParams& sp);
void launch_a8_live_scales(hipStream_t st, const StepRec* a8_recs, int64_t n_steps, int64_t base, int64_t slice, StepRec* live_recs);

// vbs_plan.cpp
struct StreamPlanIn {
    int64_t cols, w, br0, br1, jab_lo, mab_lo;
    const int64_t* row_part; const int64_t* nzcount; const int64_t* jab; const float* mab;
    int32_t dtype, n_cus;                     // n_cus: compute units of the handle's device (the host builders make no HIP call)
    const uint8_t* skip;                      // [br1 - br0] block-rows handled by the sparse-row path (no tiles), or nullptr
    bool updatable = false;                   // SPARTA_CREATE_UPDATABLE: record the source of every 16-bit slice (StreamPlanHost::upd_map / upd_hub)
    bool allow_pack = false;                  // fp32 handles made without creation flags: the one-tile plan may become a packed plan (k_f32_packed.hip)
};
struct StreamPlanHost {
    std::vector<StepRec> steps[2];            // per tile type: [0] <= 32 rows, [1] 33..64 rows
    std::vector<int32_t> wrange[2];           // [2 * n_workers] begin / end step of every worker
    std::vector<FixRec> fix;                  // split tiles + tiles of block-rows without blocks (zero fill)
    std::vector<std::pair<int64_t, int64_t>> zero_ranges;   // (first row, rows) of long block-rows without blocks: vbs_zero_rows_kernel instead of fix-up tiles
    std::vector<int32_t> fix_slots;
    std::vector<uint16_t> a16_steps[2];       // 16-bit handles: A as TM x kp slices ([k chunk of 8][row][8]), one per step, in STEP order; device image = [0] then [1]
    int n_workers = 0, n_split = 0;
    int plan_aligned[2] = {0, 0};
    bool wide16 = false;                      // 16-bit one-tile plan with two sub-workers per workgroup (2 x n_workers ranges in wrange[0])
    bool window_plan = false;                 // 64-row tiles dealt as (window, tile) pieces (SPARTA_TILE_WINDOW_COLS, experiment)
    int64_t kp = SK_KP;
    int64_t n_plan_tiles[2] = {0, 0};         // tiles (with at least one block) per plan: steps per tile decides the cache policy of the C stores
    bool tiles_row_aligned[2] = {true, true}; // every tile of the plan starts at a multiple of 32 rows of C (whole 128-byte lines of a column-major C)
    std::vector<float> a_frag;                // fp32 one-tile plan: A per step in MFMA fragment order (vbs_spmm_f32_direct_kernel), or empty
    // packed plan (fp32 one-tile plan, vbs_spmm_f32_packed_kernel): the blocks of every segment of a tile packed into shared steps.  Either a_frag or a_pack is built.
    std::vector<StepRec> psteps;              // packed steps in execution order (same workers, segments, slots and fix-up records as steps[0])
    std::vector<int32_t> pwrange;             // [2 * n_workers] begin / end packed step of every worker
    std::vector<float> a_pack;                // per packed step: [8 x int32 B row of the slot, padding][fragments], kAFragSlice floats; empty: not a packed handle
    std::vector<PackLoc> pack_loc;            // per step of steps[0] (= block): where its groups sit in a_pack
    int64_t pack_slots = 0;                   // non-empty groups = MFMA pairs of the packed plan
    // hub plan (16-bit handles of 64-wide blocks): the long tiles of 33..64 rows, grouped by the similarity of their block columns into group tiles for
    // vbs_spmm_h16_hub_kernel (k_hub16.hip); their block-rows are in none of the two plans above
    std::vector<HubStep> hub_steps;           // in execution order, padded by 32 harmless copies
    std::vector<HubTile> hub_tiles;
    std::vector<int32_t> hub_wrange;          // [2 * hub_workers]
    std::unique_ptr<uint16_t[]> hub_a16;      // slices of 64 rows x 64 k in the kernel's LDS image, present sub-tiles of a step back to back, steps in execution order
    size_t hub_a16_elems = 0;                 // (uninitialised storage: 10^10 elements on a dense hub part -- the packing loop writes every element, zeros included)
    int hub_g = 0;                            // sub-tiles per group tile (2 or 4); 0: no hub plan
    int hub_workers = 0;
    int64_t n_hub_steps = 0, hub_area = 0, hub_union_area = 0;    // steps; stored elements of the hub tiles; elements the kernel multiplies (absent sub-tiles included)
    int64_t n_hub_tiles = 0, n_hub_groups = 0, hub_chunks = 0, hub_segments = 0;    // K chunks of the step order; segments (runs of one group on one worker)
    // updatable 16-bit handles: where every slice of a16_steps[ty] / hub_a16 comes from, in image order (sparta_vbs_set_values)
    std::vector<UpdSlice> upd_map[2];
    std::vector<UpdSlice> upd_hub;
};
// vbs_union.cpp: the device form of the column-compacted tiles -- tiles dealt to workers longest first, a worker's steps back to back
struct UnionDevPlan {
    std::vector<UnionRec> rec[kUnionTypes];
    std::vector<int32_t> ids[kUnionTypes];
    std::vector<float> a[kUnionTypes];        // fp32 handles: slices [step][R x 32 + kUnionPairFloats] floats (R = 16 (type + 1)), the layout of UnionSide::A
    std::vector<uint16_t> a16[kUnionTypes];   // 16-bit handles: slices [step][R x 32] 16-bit elements (R = 32 (type + 1)), rounded to the storage type
    std::vector<int32_t> wrange[kUnionTypes];
    std::vector<uint32_t> tail[kUnionTypes];  // (column, value bits) pairs, tile after tile in execution order
    int32_t n_workers[kUnionTypes] = {0, 0, 0, 0};
    int64_t n_steps[kUnionTypes] = {0, 0, 0, 0}, n_tiles[kUnionTypes] = {0, 0, 0, 0};
    int32_t type_rows[kUnionTypes] = {0, 0, 0, 0};   // R of each type
    int64_t tiles_by_height[2] = {0, 0}, steps_by_height[2] = {0, 0};   // tiles / steps of tiles of <= 32 rows, of 33..64 rows (what sparta_vbs_union_info reports)
    int64_t area = 0, cols = 0, rows = 0;     // stored elements (tile rows x list entries); list entries; rows of C the tiles own
};
int build_union_plan(const sparta::UnionPlanHost& U, int max_workers, UnionDevPlan& P, int dtype = SPARTA_F32, int n_cus = 0);
// y (+)= the tiles' part of A . x, walked on the HOST from the device form (test aid for the CPU suite: the layout of plan and slices without a GPU)
void union_plan_host_apply(const UnionDevPlan& P, const float* x, double* y);

constexpr int64_t kZeroRangeRows = 2048;    // block-rows without blocks at least this tall are zero-filled by vbs_zero_rows_kernel
int build_stream_plans(const StreamPlanIn& in, StreamPlanHost& P);
// the block-column index of sparta_vbs_spmm_t for the block-rows [br0, br1) (jab: the whole array, jab_lo its offset of block-row br0); h16: offsets into the
// 16-bit image (and the `src` records), else into mab from the range's first element
struct SpmmTIndexHost {
    std::vector<SpmmTBlock> blocks;
    std::vector<SpmmTItem> items;
    std::vector<SpmmTSrc> src;                // h16 only, mab order
    int64_t image_elems = 0;                  // h16 only
    int64_t cols_with_blocks = 0, max_list = 0;
};
int build_spmm_t_index(int64_t cols, int64_t w, int64_t br0, int64_t br1, const int64_t* row_part, const int64_t* nzcount, const int64_t* jab, int64_t jab_lo, bool h16,
                       SpmmTIndexHost& T);
// the host forms of creation (vbs_capi.cpp: one builder and one upload per family)
// The sparse rows in the form the kernels of k_sparse.hip take them: a CSR of the rows, the short rows as a list (one wave each), the long ones cut into segments
struct SparseRowsHost {
    std::vector<uint8_t> flag;                // [br1 - br0] 1: the block-row gets no tile (StreamPlanIn::skip); empty: none does
    std::vector<int64_t> rowptr;
    std::vector<int32_t> col, crow;           // crow: the row of C of every sparse row; bit 31: the row ADDS to C (a mixed block-row's sparse part)
    std::vector<float> val;
    std::vector<int32_t> list;                // the short rows
    std::vector<SpSegRec> segs;               // the segments of the long rows in the order the waves take them; pad = the segment's index in row order
    std::vector<SpLongRec> longs;
    std::vector<int32_t> stream_begin;        // XCD order: [9] the eight streams of segs; empty: one list
    int64_t seg = 0, long_cut = 0, minseg = 0, win_w = 0;   // as order_sparse_rows resolved them: base segment length, longest short row, SPARTA_SP_MINSEG, window width (0: off)
};
// the resident-column image (k_colres.hip) of sparse rows
constexpr int64_t kColresCells = 160 * 1024 / 4;                  // floats of LDS a workgroup may hold
struct ColresHost {
    std::vector<uint16_t> col;                                    // per batch of 4 steps and lane: four columns (relative to their K range) ...
    std::vector<float> val;                                       // ... and four values (empty: every stored value is 1.0f -- a unit image, the reference's -P 1)
    std::vector<ColresPartDev> parts;
    std::vector<int32_t> meta, dest;                              // per part: see ColresPartDev
    std::vector<uint8_t> mode;                                    // per row of C (padded to 4): 0 not this kernel's, 1 store, 2 add
    std::vector<ColresLong> longs;
    std::vector<int32_t> krange;                                  // [n_ranges + 1]
    int32_t max_slices = 0, max_cells = 0, lmax = 0;              // slices of the part with most; cells a column set needs in LDS (largest range of B + its zero cell / largest staging image)
    int64_t entries = 0;
};
// what a handle keeps: the main image and, where eligible, the four-part image (SPARTA_COLRES_SMALL=0: not built)
struct ColresImages { ColresHost main, small; bool has_main = false, has_small = false; };
// the row tiles of every class in launch order (padded to 8 streams), the block-row descriptors, and the elements the tile kernels multiply
struct ClassTilesHost {
    std::vector<TileDesc> tiles[4];
    int64_t n_real[4] = {0, 0, 0, 0};
    std::vector<BlockRowDesc> brows;
    int64_t exec_area = 0;
};
// the transposed index with, for 16-bit handles, the [ceil(h / 8)][w][8] image of k_spmm_t.hip
struct SpmmTHost {
    SpmmTIndexHost index;
    std::unique_ptr<uint16_t[]> image;       // index.image_elems elements, or null
};
// the block table of block pruning: [n_blocks][4] = {offset, n_in, n_all, (block-row - br0) << 32 | block column}; table == nullptr only counts
int build_block_table(int64_t cols, int64_t w, int64_t br0, int64_t br1, const int64_t* row_part, const int64_t* nzcount, const int64_t* jab, int64_t jab_lo,
                      int64_t* table, int64_t* n_blocks);
// the pattern-only maps of the live-block set for the block-rows [br0, br1): goff[block_rows + 1] = first position of every block-row's slice of the SDDMM group
// list (a block-row of height 0 has no groups), tptr[block columns + 1] = every block column's slice of the spmm_t list (the ptr of build_spmm_t_index), tmap =
// list position -> block number (mab order, as build_block_table numbers them); and the rule itself on the host (what k_live.hip computes)
struct LiveMapsHost {
    std::vector<int64_t> goff, tptr, first_block;             // first_block[block_rows + 1]: block number of every block-row's first block
    std::vector<int32_t> tmap;
    int64_t w = 0;
};
int build_live_maps(int64_t cols, int64_t w, int64_t br0, int64_t br1, const int64_t* row_part, const int64_t* nzcount, const int64_t* jab, int64_t jab_lo, LiveMapsHost& M);
void live_lists_host(const LiveMapsHost& M, const uint8_t* keep, int32_t* sd_groups, int32_t* sd_count, int32_t* t_blocks, int32_t* t_count, int64_t* info);
// the pattern-only map of the live words of the steps' image kernels: word i covers the `span` stored columns (leading dimension ld[i]) that start at element
// first[i] of the range's mab (first[i] < 0: a slice half that is not there, wmap[i] = -1); wmap[i] = the number of the block they lie in, by the block table's
// offsets (block_off[n_blocks], ascending, mab order).  SPARTA_ERR_INVALID if a word's first and last column lie in different blocks: the image kernels test one
// bit per lane, which is right only where a step / slice half never leaves its block (block widths that are multiples of 32: every plan with an image kernel)
// live forward: the end of every step's segment, and the compaction rule on the host (what vbs_fwdlive_compact_kernel computes), see vbs_plan.cpp
void live_forward_segments(const StepRec* steps, int64_t n_steps, const int32_t* ranges, int64_t n_ranges, int32_t* seg_last);
void live_forward_compact_host(const StepRec* steps, int64_t n_steps, const int32_t* ranges, int64_t n_ranges, bool pair, const uint8_t* live, StepRec* out,
                               int32_t* ranges_out, int64_t* info);
int build_live_word_map(const int64_t* block_off, int64_t n_blocks, int64_t nztot, const int64_t* first, const int32_t* ld, int64_t n_words, int64_t span, int32_t* wmap);
// one block of the 16-bit image from its column-major h x w source
void pack_spmm_t_block(const float* blk, int64_t h, int64_t w, bool bf16, uint16_t* dst);
uint16_t to_h16(float v, bool bf16);   // fp32 -> fp16 / bf16 bits, round to nearest even (what the device conversion kernel does too)

}  // namespace sparta_dev
