// k_dense.hip -- a dense matrix and the stored blocks of a VBS handle (sparta_dense_block_ssq / sparta_vbs_gather_dense / sparta_vbs_scatter_dense,
// include/sparta_amd.h).  D is the caller's rows x cols matrix (fp32, fp16 or bf16; row- or column-major with a leading dimension), T the caller's nztot
// floats in the mab layout.  Every name starts with "vbs_dense_" and holds none of the strings the tests count the other kernels by:
//   vbs_dense_gather_rm_kernel / vbs_dense_scatter_rm_kernel   row-major D: a block is a transposition (contiguous along q in D, along i in T), staged through LDS
//   vbs_dense_gather_cm_kernel / vbs_dense_scatter_cm_kernel   column-major D: a stored column is a run of h elements on both sides, no LDS
//   vbs_dense_fill_kernel                                       the rows x cols region of D stored as +0 (all zero bits in every type), the ld padding kept
//   vbs_dense_ssq_kernel                                        per block of the (row_part, w) grid the fp64 sum of the exact squares of its elements
// The scheme of k_prune.hip and k_repattern.hip: one WAVE per work item, kPruneWaves items per workgroup, no atomics, no barrier, no cross-wave step.  A work
// item of the four copy kernels is a chunk of at most 64 rows of one stored block (DenseItem, vbs_device.hpp: cut on the host, so a block 257 rows tall is
// five items); an item of the score kernel is one grid block.  The element type and the layout of D are template arguments: no per-element branch on them.
// Element values travel as uint32 bit patterns (fp32: the word itself; bf16: << 16; fp16: the exact conversion), so no float instruction sees a payload of an
// fp32 D.  Accesses: 16 bytes per lane where the addresses of a whole tile allow it (a uniform test of base, leading dimension, height and width), one
// element per lane elsewhere -- a misaligned vector pointer is never dereferenced.
//
// The transposing tile: 64 rows x 32 columns of words in LDS, private to its wave, row stride 33 words.  ds_write_b32 / ds_read_b32 bank = word address mod 32,
// conflicts counted inside a 32-lane half: a row of 32 words (D side, scalar) hits banks r + 0..31, a column of 32 rows (T side, scalar) banks q + 0..31, a
// 16-byte D access of 8 lanes x 4 rows banks r + 4 c4 + e -- all conflict-free; the 16-byte T side reads rows 4 i4 + e of up to two columns per half (4-way
// at h = 64), which the global side hides: the kernels are bandwidth-bound.
#include "vbs_kernel_common.hpp"

namespace sparta_dev {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kDnRows = 64, kDnCols = 32, kDnStride = kDnCols + 1;

template <int DT> struct DnElem { typedef uint16_t type; };
template <> struct DnElem<SPARTA_F32> { typedef uint32_t type; };

// an element of D as the bits of the fp32 that T holds
template <int DT>
__device__ __forceinline__ uint32_t dn_widen(uint32_t x) {
    if constexpr (DT == SPARTA_F32) return x;
    else if constexpr (DT == SPARTA_BF16) return x << 16;
    else return __float_as_uint((float)__builtin_bit_cast(_Float16, (uint16_t)x));
}
// the bits of an fp32 of T as an element of D: the rounding of creation and of every image (upd_h16)
template <int DT>
__device__ __forceinline__ uint32_t dn_narrow(uint32_t bits) {
    if constexpr (DT == SPARTA_F32) return bits;
    else return upd_h16<DT == SPARTA_BF16>(__uint_as_float(bits));
}

// LDS writes of the wave are complete and no access moves across (one tile per wave: no barrier)
__device__ __forceinline__ void dn_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// lanes along a run of n (1 .. 64) elements: the power of two at or above n, as a shift
__device__ __forceinline__ int dn_shift(int n) { return n <= 1 ? 0 : 32 - __builtin_clz((unsigned)(n - 1)); }

// EPV elements of D per 16 bytes
template <int DT> constexpr int dn_epv() { return DT == SPARTA_F32 ? 4 : 8; }

// ---- row-major D -------------------------------------------------------------------------------------------------------------------------------
// D side, 16-byte form: a lane owns EPV consecutive columns of one row, 32 / EPV lanes span the tile's 32 columns, 8 (fp32) or 16 rows per instruction.
// D side, element form: a lane owns one column, the two halves of the wave two consecutive rows.
// T side, 16-byte form: a lane owns rows 4 i4 .. 4 i4 + 3 of one column; element form: one row of one column; the lanes a chunk's height leaves over take
// further columns.
template <int DT>
__global__ __launch_bounds__(kThreads) void vbs_dense_gather_rm_kernel(const DenseItem* __restrict__ items, int64_t n_items, const void* __restrict__ Dv, int64_t ldd, int w,
                                                                      uint32_t* __restrict__ T) {
    __shared__ uint32_t lds[kPruneWaves][kDnRows * kDnStride];
    typedef typename DnElem<DT>::type E;
    constexpr int EPV = dn_epv<DT>(), LPR = kDnCols / EPV, RPI = 64 / LPR;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * kPruneWaves + wave;
    if (it >= n_items) return;                  // (the whole wave)
    const DenseItem m = items[it];
    uint32_t* tile = lds[wave];
    const E* D = reinterpret_cast<const E*>(Dv) + (int64_t)(m.r0 + m.i0) * ldd + m.c0;
    uint32_t* Tb = T + m.off + m.i0;
    const int hc = m.hc;
    const int64_t h = m.h;
    const bool t_vec = (h & 3) == 0 && (hc & 3) == 0 && ((uintptr_t)Tb & 15u) == 0;
    const bool ld_vec = ((uint64_t)ldd * sizeof(E)) % 16 == 0;
    const int tsh = t_vec ? dn_shift(hc >> 2) : dn_shift(hc);
    const int ti = lane & ((1 << tsh) - 1), tq = lane >> tsh, tstep = 64 >> tsh;
    for (int c = 0; c < w; c += kDnCols) {
        const int tw = w - c < kDnCols ? w - c : kDnCols;                                  // stored columns of the tile
        const int vw = m.valid - c < 0 ? 0 : (m.valid - c < kDnCols ? m.valid - c : kDnCols);   // ... inside the matrix
        if (vw == kDnCols && ld_vec && ((uintptr_t)(D + c) & 15u) == 0) {
            const int cv = lane % LPR, rv = lane / LPR;
            for (int r = rv; r < hc; r += 4 * RPI) {
                u32x4 x[4];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (r + u * RPI < hc) x[u] = *reinterpret_cast<const u32x4*>(D + (int64_t)(r + u * RPI) * ldd + c + cv * EPV);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (r + u * RPI >= hc) continue;
                    uint32_t* dst = tile + (r + u * RPI) * kDnStride + cv * EPV;
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        if constexpr (DT == SPARTA_F32) dst[e] = x[u][e];
                        else { dst[2 * e] = dn_widen<DT>(x[u][e] & 0xffffu); dst[2 * e + 1] = dn_widen<DT>(x[u][e] >> 16); }
                    }
                }
            }
        } else if (vw > 0) {
            const int col = lane & 31, rs = lane >> 5;
            for (int r = rs; r < hc; r += 8) {
                uint32_t x[4];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (r + 2 * u < hc && col < vw) x[u] = D[(int64_t)(r + 2 * u) * ldd + c + col];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (r + 2 * u < hc && col < vw) tile[(r + 2 * u) * kDnStride + col] = dn_widen<DT>(x[u]);
            }
        }
        dn_wave_sync();
        if (t_vec) {
            if (4 * ti < hc)
                for (int q = tq; q < tw; q += tstep) {
                    u32x4 x = {0u, 0u, 0u, 0u};
                    if (q < vw) {
#pragma unroll
                        for (int e = 0; e < 4; e++) x[e] = tile[(4 * ti + e) * kDnStride + q];
                    }
                    *reinterpret_cast<u32x4*>(Tb + (int64_t)(c + q) * h + 4 * ti) = x;
                }
        } else if (ti < hc) {
            for (int q = tq; q < tw; q += tstep) Tb[(int64_t)(c + q) * h + ti] = q < vw ? tile[ti * kDnStride + q] : 0u;
        }
        dn_wave_sync();
    }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void vbs_dense_scatter_rm_kernel(const DenseItem* __restrict__ items, int64_t n_items, const uint32_t* __restrict__ T, void* __restrict__ Dv,
                                                                       int64_t ldd) {
    __shared__ uint32_t lds[kPruneWaves][kDnRows * kDnStride];
    typedef typename DnElem<DT>::type E;
    constexpr int EPV = dn_epv<DT>(), LPR = kDnCols / EPV, RPI = 64 / LPR;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * kPruneWaves + wave;
    if (it >= n_items) return;                  // (the whole wave)
    const DenseItem m = items[it];
    uint32_t* tile = lds[wave];
    E* D = reinterpret_cast<E*>(Dv) + (int64_t)(m.r0 + m.i0) * ldd + m.c0;
    const uint32_t* Tb = T + m.off + m.i0;
    const int hc = m.hc;
    const int64_t h = m.h;
    const bool t_vec = (h & 3) == 0 && (hc & 3) == 0 && ((uintptr_t)Tb & 15u) == 0;
    const bool ld_vec = ((uint64_t)ldd * sizeof(E)) % 16 == 0;
    const int tsh = t_vec ? dn_shift(hc >> 2) : dn_shift(hc);
    const int ti = lane & ((1 << tsh) - 1), tq = lane >> tsh, tstep = 64 >> tsh;
    for (int c = 0; c < m.valid; c += kDnCols) {                                           // (the stored columns past cols are not read)
        const int vw = m.valid - c < kDnCols ? m.valid - c : kDnCols;
        if (t_vec) {
            if (4 * ti < hc)
                for (int q = tq; q < vw; q += 4 * tstep) {
                    u32x4 x[4];
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (q + u * tstep < vw) x[u] = *reinterpret_cast<const u32x4*>(Tb + (int64_t)(c + q + u * tstep) * h + 4 * ti);
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (q + u * tstep < vw) {
#pragma unroll
                            for (int e = 0; e < 4; e++) tile[(4 * ti + e) * kDnStride + q + u * tstep] = x[u][e];
                        }
                }
        } else if (ti < hc) {
            for (int q = tq; q < vw; q += 4 * tstep) {
                uint32_t x[4];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (q + u * tstep < vw) x[u] = Tb[(int64_t)(c + q + u * tstep) * h + ti];
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (q + u * tstep < vw) tile[ti * kDnStride + q + u * tstep] = x[u];
            }
        }
        dn_wave_sync();
        if (vw == kDnCols && ld_vec && ((uintptr_t)(D + c) & 15u) == 0) {
            const int cv = lane % LPR, rv = lane / LPR;
            for (int r = rv; r < hc; r += RPI) {
                const uint32_t* src = tile + r * kDnStride + cv * EPV;
                u32x4 x;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    if constexpr (DT == SPARTA_F32) x[e] = src[e];
                    else x[e] = dn_narrow<DT>(src[2 * e]) | (dn_narrow<DT>(src[2 * e + 1]) << 16);
                }
                *reinterpret_cast<u32x4*>(D + (int64_t)r * ldd + c + cv * EPV) = x;
            }
        } else {
            const int col = lane & 31, rs = lane >> 5;
            if (col < vw)
                for (int r = rs; r < hc; r += 2) D[(int64_t)r * ldd + c + col] = (E)dn_narrow<DT>(tile[r * kDnStride + col]);
        }
        dn_wave_sync();
    }
}

// ---- column-major D: stored column q of a chunk is hc contiguous elements on both sides ------------------------------------------------------------
// 4-element form (a lane owns rows 4 i4 .. 4 i4 + 3 of one column: 16 bytes of T, 16 or 8 bytes of D) where height, bases and the leading dimension
// allow it; element form elsewhere.  Four loads in flight per lane.
template <int DT>
__global__ __launch_bounds__(kThreads) void vbs_dense_gather_cm_kernel(const DenseItem* __restrict__ items, int64_t n_items, const void* __restrict__ Dv, int64_t ldd, int w,
                                                                      uint32_t* __restrict__ T) {
    typedef typename DnElem<DT>::type E;
    const int lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * kPruneWaves + (threadIdx.x >> 6);
    if (it >= n_items) return;                  // (the whole wave)
    const DenseItem m = items[it];
    const E* D = reinterpret_cast<const E*>(Dv) + (int64_t)m.c0 * ldd + m.r0 + m.i0;
    uint32_t* Tb = T + m.off + m.i0;
    const int hc = m.hc, valid = m.valid;
    const int64_t h = m.h;
    const bool vec = (h & 3) == 0 && (hc & 3) == 0 && ((uintptr_t)Tb & 15u) == 0 && ((uintptr_t)D % (4 * sizeof(E))) == 0 && (ldd & 3) == 0;
    const int tsh = vec ? dn_shift(hc >> 2) : dn_shift(hc);
    const int ti = lane & ((1 << tsh) - 1), tq = lane >> tsh, tstep = 64 >> tsh;
    if (vec) {
        if (4 * ti >= hc) return;
        for (int q = tq; q < w; q += 4 * tstep) {
            u32x4 x[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int qq = q + u * tstep;
                x[u] = u32x4{0u, 0u, 0u, 0u};
                if (qq < valid) {
                    if constexpr (DT == SPARTA_F32) x[u] = *reinterpret_cast<const u32x4*>(D + (int64_t)qq * ldd + 4 * ti);
                    else {
                        const u32x2 p = *reinterpret_cast<const u32x2*>(D + (int64_t)qq * ldd + 4 * ti);
                        x[u] = u32x4{dn_widen<DT>(p[0] & 0xffffu), dn_widen<DT>(p[0] >> 16), dn_widen<DT>(p[1] & 0xffffu), dn_widen<DT>(p[1] >> 16)};
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (q + u * tstep < w) *reinterpret_cast<u32x4*>(Tb + (int64_t)(q + u * tstep) * h + 4 * ti) = x[u];
        }
    } else {
        if (ti >= hc) return;
        for (int q = tq; q < w; q += 4 * tstep) {
            uint32_t x[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int qq = q + u * tstep;
                x[u] = 0u;
                if (qq < valid) x[u] = dn_widen<DT>(D[(int64_t)qq * ldd + ti]);
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (q + u * tstep < w) Tb[(int64_t)(q + u * tstep) * h + ti] = x[u];
        }
    }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void vbs_dense_scatter_cm_kernel(const DenseItem* __restrict__ items, int64_t n_items, const uint32_t* __restrict__ T, void* __restrict__ Dv,
                                                                       int64_t ldd) {
    typedef typename DnElem<DT>::type E;
    const int lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * kPruneWaves + (threadIdx.x >> 6);
    if (it >= n_items) return;                  // (the whole wave)
    const DenseItem m = items[it];
    E* D = reinterpret_cast<E*>(Dv) + (int64_t)m.c0 * ldd + m.r0 + m.i0;
    const uint32_t* Tb = T + m.off + m.i0;
    const int hc = m.hc, valid = m.valid;
    const int64_t h = m.h;
    const bool vec = (h & 3) == 0 && (hc & 3) == 0 && ((uintptr_t)Tb & 15u) == 0 && ((uintptr_t)D % (4 * sizeof(E))) == 0 && (ldd & 3) == 0;
    const int tsh = vec ? dn_shift(hc >> 2) : dn_shift(hc);
    const int ti = lane & ((1 << tsh) - 1), tq = lane >> tsh, tstep = 64 >> tsh;
    if (vec) {
        if (4 * ti >= hc) return;
        for (int q = tq; q < valid; q += 4 * tstep) {                                     // (the stored columns past cols are not read)
            u32x4 x[4];
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (q + u * tstep < valid) x[u] = *reinterpret_cast<const u32x4*>(Tb + (int64_t)(q + u * tstep) * h + 4 * ti);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int qq = q + u * tstep;
                if (qq >= valid) continue;
                if constexpr (DT == SPARTA_F32) *reinterpret_cast<u32x4*>(D + (int64_t)qq * ldd + 4 * ti) = x[u];
                else
                    *reinterpret_cast<u32x2*>(D + (int64_t)qq * ldd + 4 * ti) =
                        u32x2{dn_narrow<DT>(x[u][0]) | (dn_narrow<DT>(x[u][1]) << 16), dn_narrow<DT>(x[u][2]) | (dn_narrow<DT>(x[u][3]) << 16)};
            }
        }
    } else {
        if (ti >= hc) return;
        for (int q = tq; q < valid; q += 4 * tstep) {
            uint32_t x[4];
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (q + u * tstep < valid) x[u] = Tb[(int64_t)(q + u * tstep) * h + ti];
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (q + u * tstep < valid) D[(int64_t)(q + u * tstep) * ldd + ti] = (E)dn_narrow<DT>(x[u]);
        }
    }
}

// ---- fill: n_runs runs of run_bytes bytes, ld_bytes apart, stored as zero bytes (+0 of every type) -------------------------------------------------
// A thread owns one 16-byte cell of the run's own 16-byte grid: a cell inside the run is one 16-byte store, the cells the run's ends cut are stored element
// by element (ESZ bytes each; a run starts and ends on an element boundary).  Workgroup b: run b / segs, cells 256 (b % segs) .. + 255.
template <int ESZ>
__global__ __launch_bounds__(kThreads) void vbs_dense_fill_kernel(uint8_t* D, int64_t ld_bytes, int64_t run_bytes, int64_t segs) {
    const int64_t run = (int64_t)blockIdx.x / segs, seg = (int64_t)blockIdx.x - run * segs;
    const uintptr_t a = (uintptr_t)D + (uintptr_t)(run * ld_bytes), end = a + (uintptr_t)run_bytes;
    const uintptr_t cell = (a & ~(uintptr_t)15) + (uintptr_t)((seg * kThreads + threadIdx.x) * 16);
    if (cell >= end) return;
    if (cell >= a && cell + 16 <= end) {
        *reinterpret_cast<u32x4*>(cell) = u32x4{0u, 0u, 0u, 0u};
        return;
    }
    const uintptr_t lo = cell < a ? a : cell, hi = cell + 16 < end ? cell + 16 : end;
    for (uintptr_t p = lo; p < hi; p += ESZ) {
        if constexpr (ESZ == 4) *reinterpret_cast<uint32_t*>(p) = 0u;
        else *reinterpret_cast<uint16_t*>(p) = (uint16_t)0;
    }
}

// ---- the grid score ----------------------------------------------------------------------------------------------------------------------------------
// One wave per block (ib, jb) of the grid.  Its elements are n_run runs of run_len contiguous elements, ldd apart: the block's rows (row-major) or its columns
// (column-major).  lp = the power of two at or above min(run_len, 64) lanes walk a run, 64 / lp runs per instruction.  A lane's elements in a fixed order: its
// runs four at a time, run u of the four into accumulator u (four loads in flight), the runs left over into the first; accumulators summed 0..3; lanes by
// xor-shuffle.  pr_fold of k_prune.hip: the square is exact in fp64, the FMA rounds once.  row_part is read here and clamped into [0, rows]: whatever it
// holds, nothing outside D is read.
template <int DT, bool RM>
__global__ __launch_bounds__(kThreads) void vbs_dense_ssq_kernel(const void* __restrict__ Dv, int64_t ldd, int64_t rows, int64_t cols, int64_t n_grid, int64_t block_cols, int64_t w,
                                                                const int64_t* __restrict__ row_part, double* __restrict__ ssq_out) {
    typedef typename DnElem<DT>::type E;
    const int64_t b = (int64_t)blockIdx.x * kPruneWaves + (threadIdx.x >> 6);
    if (b >= n_grid) return;                    // (the whole wave)
    const int lane = threadIdx.x & 63;
    const int64_t ib = b / block_cols, jb = b - ib * block_cols;
    int64_t r0 = row_part[ib], r1 = row_part[ib + 1];
    r0 = r0 < 0 ? 0 : (r0 > rows ? rows : r0);
    r1 = r1 < r0 ? r0 : (r1 > rows ? rows : r1);
    const int64_t c0 = jb * w, valid = cols - c0 < w ? cols - c0 : w, h = r1 - r0;
    const int64_t run_len = RM ? valid : h, n_run = RM ? h : valid;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (run_len > 0 && n_run > 0) {
        const E* p = reinterpret_cast<const E*>(Dv) + (RM ? r0 * ldd + c0 : c0 * ldd + r0);
        const int sh = run_len >= 64 ? 6 : dn_shift((int)run_len), lp = 1 << sh;
        const int64_t e0 = lane & (lp - 1), R = 64 >> sh;
        int64_t run = lane >> sh;
        for (; run + 3 * R < n_run; run += 4 * R)
            for (int64_t e = e0; e < run_len; e += lp) {
                uint32_t x[4];
#pragma unroll
                for (int u = 0; u < 4; u++) x[u] = p[(run + u * R) * ldd + e];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const double d = (double)__uint_as_float(dn_widen<DT>(x[u]));
                    acc[u] = fma(d, d, acc[u]);
                }
            }
        for (; run < n_run; run += R)
            for (int64_t e = e0; e < run_len; e += lp) {
                const double d = (double)__uint_as_float(dn_widen<DT>(p[run * ldd + e]));
                acc[0] = fma(d, d, acc[0]);
            }
    }
    double s = ((acc[0] + acc[1]) + acc[2]) + acc[3];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) ssq_out[b] = s;
}

unsigned dn_grid(int64_t n) { return (unsigned)((n + kPruneWaves - 1) / kPruneWaves); }

}  // namespace

void launch_dense_gather(hipStream_t st, const DenseItem* items, int64_t n_items, const void* D, int64_t ldd, int row_major, int dtype, int w, float* T) {
    uint32_t* t = reinterpret_cast<uint32_t*>(T);
    const dim3 g(dn_grid(n_items)), b(kThreads);
#define SPARTA_DN_GATHER(DT)                                                                                                   \
    if (row_major) hipLaunchKernelGGL(vbs_dense_gather_rm_kernel<DT>, g, b, 0, st, items, n_items, D, ldd, w, t);               \
    else hipLaunchKernelGGL(vbs_dense_gather_cm_kernel<DT>, g, b, 0, st, items, n_items, D, ldd, w, t)
    if (dtype == SPARTA_F32) { SPARTA_DN_GATHER(SPARTA_F32); }
    else if (dtype == SPARTA_F16) { SPARTA_DN_GATHER(SPARTA_F16); }
    else { SPARTA_DN_GATHER(SPARTA_BF16); }
#undef SPARTA_DN_GATHER
}

void launch_dense_scatter(hipStream_t st, const DenseItem* items, int64_t n_items, const float* T, void* D, int64_t ldd, int row_major, int dtype) {
    const uint32_t* t = reinterpret_cast<const uint32_t*>(T);
    const dim3 g(dn_grid(n_items)), b(kThreads);
#define SPARTA_DN_SCATTER(DT)                                                                                                  \
    if (row_major) hipLaunchKernelGGL(vbs_dense_scatter_rm_kernel<DT>, g, b, 0, st, items, n_items, t, D, ldd);                 \
    else hipLaunchKernelGGL(vbs_dense_scatter_cm_kernel<DT>, g, b, 0, st, items, n_items, t, D, ldd)
    if (dtype == SPARTA_F32) { SPARTA_DN_SCATTER(SPARTA_F32); }
    else if (dtype == SPARTA_F16) { SPARTA_DN_SCATTER(SPARTA_F16); }
    else { SPARTA_DN_SCATTER(SPARTA_BF16); }
#undef SPARTA_DN_SCATTER
}

// workgroups of the fill: per run the 16-byte cells of run_bytes + at most 15 bytes in front of it, kThreads cells per workgroup
int64_t dense_fill_segs(int64_t run_bytes) { return (run_bytes + 15 + 16 * kThreads - 1) / (16 * kThreads); }

void launch_dense_fill(hipStream_t st, void* D, int64_t ldd, int row_major, int dtype, int64_t rows, int64_t cols) {
    const int64_t esz = dtype == SPARTA_F32 ? 4 : 2, n_runs = row_major ? rows : cols, run_bytes = (row_major ? cols : rows) * esz, segs = dense_fill_segs(run_bytes);
    const dim3 g((unsigned)(n_runs * segs)), b(kThreads);
    if (esz == 4) hipLaunchKernelGGL(vbs_dense_fill_kernel<4>, g, b, 0, st, (uint8_t*)D, ldd * esz, run_bytes, segs);
    else hipLaunchKernelGGL(vbs_dense_fill_kernel<2>, g, b, 0, st, (uint8_t*)D, ldd * esz, run_bytes, segs);
}

void launch_dense_block_ssq(hipStream_t st, const void* D, int64_t ldd, int row_major, int dtype, int64_t rows, int64_t cols, int64_t block_rows, int64_t w,
                            const int64_t* row_part, double* ssq_out) {
    const int64_t block_cols = (cols - 1) / w + 1, n_grid = block_rows * block_cols;
    const dim3 g(dn_grid(n_grid)), b(kThreads);
#define SPARTA_DN_SSQ(DT)                                                                                                                          \
    if (row_major) hipLaunchKernelGGL((vbs_dense_ssq_kernel<DT, true>), g, b, 0, st, D, ldd, rows, cols, n_grid, block_cols, w, row_part, ssq_out);  \
    else hipLaunchKernelGGL((vbs_dense_ssq_kernel<DT, false>), g, b, 0, st, D, ldd, rows, cols, n_grid, block_cols, w, row_part, ssq_out)
    if (dtype == SPARTA_F32) { SPARTA_DN_SSQ(SPARTA_F32); }
    else if (dtype == SPARTA_F16) { SPARTA_DN_SSQ(SPARTA_F16); }
    else { SPARTA_DN_SSQ(SPARTA_BF16); }
#undef SPARTA_DN_SSQ
}

}  // namespace sparta_dev
