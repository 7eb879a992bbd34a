// k_epilogue.hip -- the epilogue of a block-sparse linear layer (sparta_epilogue_fwd / sparta_epilogue_bwd, include/sparta_amd.h): bias, activation and the
// output type in ONE pass behind the forward product, and in ONE pass in front of the two backward products -- which also writes their operand in the handle's
// type and the bias gradient.  Handle-free: the operands are column-major rows x n_cols matrices with a leading dimension (a contiguous torch (n, rows)
// tensor IS one).  No name holds "vbs_adam_", "vbs_sgd_", "vbs_update_", "vbs_prune_", "stream_kernel", "direct_kernel", "sddmm", "gradctl" or "live" (the
// tests count the kernels of the steps, of set_values and of the products by those):
//   vbs_epilogue_fwd_kernel<TY>        Y = act(Z + bias), rounded to TY
//   vbs_epilogue_bwd_kernel<TDY, TDZ>  dZ = dY * act'(Z + bias), rounded to TDZ; per row and run of kEpRun columns the fp64 sum of the fp32 dz
//   vbs_epilogue_fold_kernel           the run sums of a row added in run order, rounded once to fp32 (only when n_cols > kEpRun, or n_cols == 0)
// Both element kernels are bandwidth-bound streams shaped as k_prune.hip's: a work item is a TILE of 256 rows x a RUN of 32 columns; wave w takes the columns
// 8 w .. 8 w + 7 of the run, four at a time with all their loads issued before the first is used.  In a BODY tile a lane owns four consecutive rows, rows
// [head + 4 g, head + 4 g + 4): one 16-byte access per fp32 operand and column (8 bytes per 16-bit operand), which the host grants only where every operand
// is aligned there in every column (ep_plan, vbs_capi.cpp: the bases agree on `head` modulo 4 elements and every leading dimension is a multiple of 4).  The
// rows in front of the body and behind it -- or ALL rows when the operands allow no common alignment -- go through EDGE tiles: lane l owns the rows l, l + 64,
// l + 128, l + 192 of the tile's 256, one element per access, still coalesced.  Owning four rows rather than eight keeps 16-bit accesses at 8 bytes, and the
// headline shape (62 464 x 128) at 976 workgroups = 3904 waves: with eight the grid would not fill 256 CUs, and the erf and exp of GELU need the waves.
// The bias gradient: every lane leaves its fp32 dz in LDS (s_dz[column of the run][row of the tile]); behind a barrier thread t sums row t over the run's
// columns in ascending order in fp64 from 0.0 -- no shuffle, no atomic, nothing that depends on the grid -- and stores the sum rounded to fp32 (one run) or as
// the run's fp64 partial part[run * rows + row], which the fold kernel adds in run order.  Offsets are 64-bit.  In place (Y == Z, dZ == dY with equal types
// and leading dimensions): a lane reads the elements it owns before it writes them, and no other lane touches them.
#include "vbs_kernel_common.hpp"

namespace sparta_dev {
namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// T: 0 = fp32, 1 = fp16, 2 = bf16 (SPARTA_F32 / F16 / BF16).  16-bit inputs are widened exactly; outputs are rounded to nearest even by upd_h16.
template <int T>
__device__ __forceinline__ float ep_widen(uint32_t h) {
    if constexpr (T == 2) return __uint_as_float(h << 16);
    else return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
}
template <int T>
__device__ __forceinline__ float ep_load1(const void* p, int64_t i) {
    if constexpr (T == 0) return reinterpret_cast<const float*>(p)[i];
    else return ep_widen<T>(reinterpret_cast<const uint16_t*>(p)[i]);
}
template <int T>
__device__ __forceinline__ f32x4 ep_load4(const void* p, int64_t i) {      // 16 bytes of fp32 / 8 bytes of a 16-bit type, aligned (ep_plan)
    if constexpr (T == 0) return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p) + i);
    else {
        const u32x2 r = *reinterpret_cast<const u32x2*>(reinterpret_cast<const uint16_t*>(p) + i);
        return f32x4{ep_widen<T>(r[0] & 0xffffu), ep_widen<T>(r[0] >> 16), ep_widen<T>(r[1] & 0xffffu), ep_widen<T>(r[1] >> 16)};
    }
}
template <int T>
__device__ __forceinline__ void ep_store1(void* p, int64_t i, float v) {
    if constexpr (T == 0) reinterpret_cast<float*>(p)[i] = v;
    else reinterpret_cast<uint16_t*>(p)[i] = (uint16_t)upd_h16<T == 2>(v);
}
template <int T>
__device__ __forceinline__ void ep_store4(void* p, int64_t i, const f32x4& v) {
    if constexpr (T == 0) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p) + i) = v;
    else
        *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(p) + i) =
            u32x2{upd_h16<T == 2>(v[0]) | (upd_h16<T == 2>(v[1]) << 16), upd_h16<T == 2>(v[2]) | (upd_h16<T == 2>(v[3]) << 16)};
}

// The arithmetic include/sparta_amd.h pins: every fp32 operation rounded once, in this order, never contracted (no fast-math flag on this file; erff and expf
// are the device library's).  The selects of ReLU pass a NaN in u and drop a NaN in dy under a masked position.
__device__ __forceinline__ float ep_fwd(float u, int act) {
#pragma clang fp contract(off)
    if (act == kEpRelu) return u <= 0.0f ? 0.0f : u;
    if (act == kEpGelu) {
        const float e = erff(u * 0.70710678f);
        const float hu = 0.5f * u;
        return hu * (1.0f + e);
    }
    return u;
}
__device__ __forceinline__ float ep_bwd(float dy, float u, int act) {
#pragma clang fp contract(off)
    if (act == kEpRelu) return u <= 0.0f ? 0.0f : dy;
    if (act == kEpGelu) {
        const float e = erff(u * 0.70710678f);
        const float cdf = 0.5f * (1.0f + e);
        const float t = (-0.5f * u) * u;
        const float pdf = (u * expf(t)) * 0.39894228f;
        return dy * (cdf + pdf);
    }
    return dy;
}

// the rows of a work item.  Body tile: lane l owns rows r0 .. r0 + 3 (slot s = row r0 + s, LDS row 4 l + s), all four or none.  Edge tile: slot s is
// element q = l + 64 s of the tile (LDS row q), edge element e = 256 * (tile - vec_tiles) + q: row e in front of the body, row e + 4 n4 behind it.
struct EpRows {
    bool vec;
    bool ok[4];
    int64_t row[4];
};
__device__ __forceinline__ bool ep_edge_row(const EpilogueParams& p, int64_t e, int64_t& row) {
    row = e < p.head ? e : e + 4 * p.n4;
    return e < p.rows - 4 * p.n4;
}
__device__ __forceinline__ EpRows ep_rows(const EpilogueParams& p, int64_t tile, int lane) {
    EpRows r;
    r.vec = tile < p.vec_tiles;
    if (r.vec) {
        const int64_t g = tile * 64 + lane;
#pragma unroll
        for (int s = 0; s < 4; s++) { r.ok[s] = g < p.n4; r.row[s] = p.head + 4 * g + s; }
    } else {
#pragma unroll
        for (int s = 0; s < 4; s++) r.ok[s] = ep_edge_row(p, (tile - p.vec_tiles) * kThreads + lane + 64 * s, r.row[s]);
    }
    return r;
}
// ... and of LDS row t of the tile, for the sums
__device__ __forceinline__ bool ep_row_of(const EpilogueParams& p, int64_t tile, int t, int64_t& row) {
    if (tile < p.vec_tiles) {
        const int64_t g = tile * 64 + (t >> 2);
        row = p.head + 4 * g + (t & 3);
        return g < p.n4;
    }
    return ep_edge_row(p, (tile - p.vec_tiles) * kThreads + t, row);
}

template <int TY>
__global__ __launch_bounds__(kThreads) void vbs_epilogue_fwd_kernel(EpilogueParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_tiles = p.vec_tiles + p.edge_tiles, total = n_tiles * p.n_runs;
    const int act = p.act;
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const int64_t tile = w % n_tiles, run = w / n_tiles;
        const EpRows r = ep_rows(p, tile, lane);
        float b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (p.bias) {
#pragma unroll
            for (int s = 0; s < 4; s++)
                if (r.ok[s]) b[s] = p.bias[r.row[s]];
        }
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int64_t c0 = run * kEpRun + wave * 8 + half * 4;
            if (c0 >= p.n_cols) break;                       // (the whole wave)
            f32x4 z[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                z[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (c0 + k >= p.n_cols) continue;
                if (r.vec) {
                    if (r.ok[0]) z[k] = ep_load4<0>(p.Z, (c0 + k) * p.ldz + r.row[0]);
                } else {
#pragma unroll
                    for (int s = 0; s < 4; s++)
                        if (r.ok[s]) z[k][s] = ep_load1<0>(p.Z, (c0 + k) * p.ldz + r.row[s]);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (c0 + k >= p.n_cols) continue;
                f32x4 y;
#pragma unroll
                for (int s = 0; s < 4; s++) {
#pragma clang fp contract(off)
                    const float u = p.bias ? z[k][s] + b[s] : z[k][s];
                    y[s] = ep_fwd(u, act);
                }
                if (r.vec) {
                    if (r.ok[0]) ep_store4<TY>(p.Out, (c0 + k) * p.ldo + r.row[0], y);
                } else {
#pragma unroll
                    for (int s = 0; s < 4; s++)
                        if (r.ok[s]) ep_store1<TY>(p.Out, (c0 + k) * p.ldo + r.row[s], y[s]);
                }
            }
        }
    }
}

template <int TDY, int TDZ>
__global__ __launch_bounds__(kThreads) void vbs_epilogue_bwd_kernel(EpilogueParams p) {
    __shared__ float s_dz[kEpRun][kThreads];                 // the fp32 dz of the work item: [column of the run][row of the tile]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n_tiles = p.vec_tiles + p.edge_tiles, total = n_tiles * p.n_runs;
    const int act = p.act;
    const bool need_u = act != kEpNone, reduce = p.dbias != nullptr;
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const int64_t tile = w % n_tiles, run = w / n_tiles;
        const EpRows r = ep_rows(p, tile, lane);
        float b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (need_u && p.bias) {
#pragma unroll
            for (int s = 0; s < 4; s++)
                if (r.ok[s]) b[s] = p.bias[r.row[s]];
        }
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int cl0 = wave * 8 + half * 4;             // column of the run
            const int64_t c0 = run * kEpRun + cl0;
            if (c0 >= p.n_cols) break;                       // (the whole wave)
            f32x4 dy[4], z[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                z[k] = dy[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (c0 + k >= p.n_cols) continue;
                if (r.vec) {
                    if (r.ok[0]) {
                        dy[k] = ep_load4<TDY>(p.dY, (c0 + k) * p.lddy + r.row[0]);
                        if (need_u) z[k] = ep_load4<0>(p.Z, (c0 + k) * p.ldz + r.row[0]);
                    }
                } else {
#pragma unroll
                    for (int s = 0; s < 4; s++)
                        if (r.ok[s]) {
                            dy[k][s] = ep_load1<TDY>(p.dY, (c0 + k) * p.lddy + r.row[s]);
                            if (need_u) z[k][s] = ep_load1<0>(p.Z, (c0 + k) * p.ldz + r.row[s]);
                        }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (c0 + k >= p.n_cols) continue;
                f32x4 dz;
#pragma unroll
                for (int s = 0; s < 4; s++) {
#pragma clang fp contract(off)
                    const float u = p.bias ? z[k][s] + b[s] : z[k][s];
                    dz[s] = ep_bwd(dy[k][s], u, act);
                }
                if (r.vec) {
                    if (r.ok[0]) {
                        ep_store4<TDZ>(p.Out, (c0 + k) * p.ldo + r.row[0], dz);
                        if (reduce) *reinterpret_cast<f32x4*>(&s_dz[cl0 + k][4 * lane]) = dz;
                    }
                } else {
#pragma unroll
                    for (int s = 0; s < 4; s++)
                        if (r.ok[s]) {
                            ep_store1<TDZ>(p.Out, (c0 + k) * p.ldo + r.row[s], dz[s]);
                            if (reduce) s_dz[cl0 + k][lane + 64 * s] = dz[s];
                        }
                }
            }
        }
        if (reduce) {                                        // (the whole grid)
            __syncthreads();
            int64_t row;
            if (ep_row_of(p, tile, (int)threadIdx.x, row)) {
                const int nc = (int)(p.n_cols - run * kEpRun < kEpRun ? p.n_cols - run * kEpRun : kEpRun);
                double sum = 0.0;
                for (int c = 0; c < nc; c++) sum += (double)s_dz[c][threadIdx.x];
                if (p.n_runs == 1) p.dbias[row] = (float)sum;
                else p.part[run * p.rows + row] = sum;
            }
            __syncthreads();
        }
    }
}

// dbias[i] = the run sums of row i added in run order, rounded once to fp32; n_runs == 0 (n_cols == 0): +0.0f
__global__ __launch_bounds__(kThreads) void vbs_epilogue_fold_kernel(const double* __restrict__ part, int64_t n_runs, int64_t rows, float* __restrict__ dbias) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < rows; i += (int64_t)gridDim.x * kThreads) {
        double sum = 0.0;
        for (int64_t r = 0; r < n_runs; r++) sum += part[r * rows + i];
        dbias[i] = (float)sum;
    }
}

// one workgroup per work item: a function of (rows, n_cols) and of the operands' alignment alone; past 2^20 workgroups they walk the items round-robin
unsigned ep_grid(const EpilogueParams& p) {
    const int64_t total = (p.vec_tiles + p.edge_tiles) * p.n_runs;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(total, 1 << 20));
}

}  // namespace

void launch_epilogue_fwd(hipStream_t st, int y_dtype, const EpilogueParams& p) {
    const dim3 grid(ep_grid(p)), block(kThreads);
    if (y_dtype == SPARTA_F32) hipLaunchKernelGGL((vbs_epilogue_fwd_kernel<0>), grid, block, 0, st, p);
    else if (y_dtype == SPARTA_F16) hipLaunchKernelGGL((vbs_epilogue_fwd_kernel<1>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((vbs_epilogue_fwd_kernel<2>), grid, block, 0, st, p);
}

template <int TDY>
static void ep_launch_bwd(hipStream_t st, int dz_dtype, const EpilogueParams& p) {
    const dim3 grid(ep_grid(p)), block(kThreads);
    if (dz_dtype == SPARTA_F32) hipLaunchKernelGGL((vbs_epilogue_bwd_kernel<TDY, 0>), grid, block, 0, st, p);
    else if (dz_dtype == SPARTA_F16) hipLaunchKernelGGL((vbs_epilogue_bwd_kernel<TDY, 1>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((vbs_epilogue_bwd_kernel<TDY, 2>), grid, block, 0, st, p);
}

void launch_epilogue_bwd(hipStream_t st, int dy_dtype, int dz_dtype, const EpilogueParams& p) {
    if (p.n_cols > 0) {
        if (dy_dtype == SPARTA_F32) ep_launch_bwd<0>(st, dz_dtype, p);
        else if (dy_dtype == SPARTA_F16) ep_launch_bwd<1>(st, dz_dtype, p);
        else ep_launch_bwd<2>(st, dz_dtype, p);
    }
    if (p.dbias && p.n_runs != 1) {
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((p.rows + kThreads - 1) / kThreads, 1 << 20));
        hipLaunchKernelGGL(vbs_epilogue_fold_kernel, dim3(grid), dim3(kThreads), 0, st, p.part, (int64_t)p.n_runs, p.rows, p.dbias);
    }
}

}  // namespace sparta_dev
