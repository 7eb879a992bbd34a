// k_spmm_t.hip -- the transposed product on the stored blocks of a VBS handle (sparta_vbs_spmm_t):
//   Ct[jb * w + q, n] (+)= sum over the blocks (ib, jb) of block column jb, sum_i A_block[i, q] * X[r0(ib) + i, n]
// the gradient of the dense operand of C = A * B (X = dC, Ct = dB).  The contraction runs over the ROWS of a block, so many block-rows add to
// the same rows of Ct: the product walks A by block column (the index of vbs_plan.cpp: build_spmm_t_index) and an output element has ONE owner.
//
// One workgroup (4 waves) per work item = (block column, panel of <= 32 of its stored columns) x one slab of 128 columns of X; wave v owns
// columns 32 v .. 32 v + 31 of the slab and walks the item's whole list of blocks with its 32 x 32 sums in 16 accumulator registers, then
// writes its piece of Ct once.  Every element of Ct is summed by one wave in list order: the same bits on every call, no atomics, no workspace.
//
// The operands are swapped as in k_sddmm.hip (MFMA "A" operand = X, M = column n of X; "B" operand = the block, N = stored column q), so
// register r of lane (q = lane & 31, g = lane >> 5) holds Ct[col(q), n0 + (r & 3) + 8 (r >> 2) + 4 g]: one store instruction writes, per half-wave,
// 32 consecutive rows of one column of the column-major Ct -- 128 contiguous bytes.
//
// Both operands are contiguous along the contraction index (a block is column-major h x w, X is column-major), so neither needs a transposing
// read or an LDS stage: a lane fetches consecutive rows with 16-byte loads straight into the registers the MFMAs consume.
//   fp32   v_mfma_f32_32x32x2_f32; a pass covers 16 rows of the block: half g of the wave takes rows 8 g .. 8 g + 7 of it (two 16-byte loads per
//          operand, 4-byte aligned), MFMA j multiplies row 8 g + j of both halves -- the order in which k is consumed is free as long as both
//          operands agree.
//   16-bit v_mfma_f32_32x32x16_{f16,bf16} on the handle's [ceil(h / 8)][w][8] image: a 16-byte chunk IS the MFMA operand of one lane (8 consecutive
//          rows of one stored column), neighbouring lanes read neighbouring chunks; the 8 rows of X are 16 contiguous bytes as well (2-byte
//          aligned: r0 is arbitrary).  A pass covers 32 rows (two MFMAs).
// The loads of the next pass (of the next block, at a block's end) are issued before the MFMAs of the current one.  Heights that are not a
// multiple of the pass, n_cols that is not a multiple of 32, narrow blocks (w < 32) and the ragged last block column are masked here: a masked
// lane loads nothing and stores nothing, a partial run of rows is loaded element by element.  Nothing is read outside a block, outside the rows
// r0 .. r0 + h - 1 of a valid column of X, and nothing is written at or beyond row `cols` or column `n_cols` of Ct.
#include "vbs_kernel_common.hpp"

namespace sparta_dev {

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8u __attribute__((ext_vector_type(8), aligned(2)));   // 2-byte aligned: 8 consecutive rows of a column of X from any row

// `rem` (> 0 where anything is to be read) elements at p are valid; the rest of the four are zeros
__device__ __forceinline__ f32x4 st_load4(const float* p, int rem, bool ok) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ok && rem >= 4) v = *reinterpret_cast<const f32x4u*>(p);
    else if (ok) {
#pragma unroll
        for (int e = 0; e < 3; e++)
            if (e < rem) v[e] = p[e];
    }
    return v;
}

__device__ __forceinline__ u16x8 st_load8(const uint16_t* p, int rem, bool ok) {
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ok && rem >= 8) v = *reinterpret_cast<const u16x8u*>(p);
    else if (ok) {
#pragma unroll
        for (int e = 0; e < 7; e++)
            if (e < rem) v[e] = p[e];
    }
    return v;
}

// the wave's 32 x 32 sums -> Ct: lane (q = lane & 31, g = lane >> 5), register r: column n0 + (r & 3) + 8 (r >> 2) + 4 g of Ct, row `col`
__device__ __forceinline__ void st_store(const f32x16& acc, float* Ct, int64_t ldo, int64_t col, bool q_ok, int n0, int n_cols, int g, int accumulate) {
    if (!q_ok) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int n = n0 + (r & 3) + 8 * (r >> 2) + 4 * g;
        if (n >= n_cols) continue;
        float* dst = Ct + col + (int64_t)n * ldo;
        *dst = accumulate ? *dst + acc[r] : acc[r];
    }
}

constexpr int kPass32 = 16;      // rows of a block per pass, fp32 (8 MFMAs of depth 2)
constexpr int kPass16 = 32;      // 16-bit (2 MFMAs of depth 16)

struct Frag32 { f32x4 a0, a1, x0, x1; };

__global__ __launch_bounds__(kThreads) void vbs_spmm_t_f32_kernel(const SpmmTParams p) {
    const SpmmTItem it = p.items[blockIdx.x];
    const int lane = threadIdx.x & 63, ql = lane & 31, g = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n0 = (int)blockIdx.y * kSpmmTSlab + 32 * wv;
    if (n0 >= p.n_cols) return;                                    // wave-uniform (no barrier in this kernel)
    const int64_t col = (int64_t)it.jb * p.w + it.q0 + ql;
    const bool q_ok = it.q0 + ql < p.w && col < p.cols;
    const bool n_ok = n0 + ql < p.n_cols;
    const float* A = (const float*)p.A;
    const float* Xn = (const float*)p.X + (int64_t)(n_ok ? n0 + ql : n0) * p.ldx;
    auto fetch = [&](const SpmmTBlock& b, int k0, Frag32& f) {
        const int kk = k0 + 8 * g, rem = b.h - kk;
        const float* ap = A + b.off + (int64_t)(it.q0 + ql) * b.h + kk;
        const float* xp = Xn + b.r0 + kk;
        f.a0 = st_load4(ap, rem, q_ok && rem > 0);
        f.a1 = st_load4(ap + 4, rem - 4, q_ok && rem > 4);
        f.x0 = st_load4(xp, rem, n_ok && rem > 0);
        f.x1 = st_load4(xp + 4, rem - 4, n_ok && rem > 4);
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    int l = it.l0, k0 = 0;
    bool have = l < it.l1;
    SpmmTBlock b = {0, 0, 0};
    Frag32 cur = {};
    if (have) { b = p.blocks[l]; fetch(b, 0, cur); }
    while (have) {
        int nl = l, nk = k0 + kPass32;
        SpmmTBlock nb = b;
        if (nk >= b.h) {
            nl = l + 1; nk = 0;
            if (nl < it.l1) nb = p.blocks[nl];
        }
        const bool nhave = nl < it.l1;
        Frag32 nxt = {};
        if (nhave) fetch(nb, nk, nxt);
#pragma unroll
        for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.x0[j], cur.a0[j], acc, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.x1[j], cur.a1[j], acc, 0, 0, 0);
        cur = nxt; b = nb; l = nl; k0 = nk; have = nhave;
    }
    st_store(acc, p.Ct, p.ldo, col, q_ok, n0, p.n_cols, g, p.accumulate);
}

struct Frag16 { u16x8 a0, a1, x0, x1; };

template <bool BF16>
__global__ __launch_bounds__(kThreads) void vbs_spmm_t_h16_kernel(const SpmmTParams p) {
    const SpmmTItem it = p.items[blockIdx.x];
    const int lane = threadIdx.x & 63, ql = lane & 31, g = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n0 = (int)blockIdx.y * kSpmmTSlab + 32 * wv;
    if (n0 >= p.n_cols) return;
    const int64_t col = (int64_t)it.jb * p.w + it.q0 + ql;
    const bool q_ok = it.q0 + ql < p.w && col < p.cols;
    const bool n_ok = n0 + ql < p.n_cols;
    const uint16_t* A = (const uint16_t*)p.A;
    const uint16_t* Xn = (const uint16_t*)p.X + (int64_t)(n_ok ? n0 + ql : n0) * p.ldx;
    auto fetch = [&](const SpmmTBlock& b, int k0, Frag16& f) {
        // MFMA m of the pass multiplies rows k0 + 16 m + 8 g .. + 7: chunk (k0 >> 3) + 2 m + g of the block (rows past h are zeros in the image)
        const int kk = k0 + 8 * g, rem = b.h - kk;
        const uint16_t* ap = A + b.off + ((int64_t)(kk >> 3) * p.w + it.q0 + ql) * 8;
        const uint16_t* xp = Xn + b.r0 + kk;
        const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        f.a0 = q_ok && rem > 0 ? *reinterpret_cast<const u16x8*>(ap) : z;
        f.a1 = q_ok && rem > 16 ? *reinterpret_cast<const u16x8*>(ap + (int64_t)p.w * 16) : z;
        f.x0 = st_load8(xp, rem, n_ok && rem > 0);
        f.x1 = st_load8(xp + 16, rem - 16, n_ok && rem > 16);
    };
    auto mma = [&](const u16x8& x, const u16x8& a, f32x16& acc) {
        if constexpr (BF16) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x), __builtin_bit_cast(bf16x8, a), acc, 0, 0, 0);
        else acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, x), __builtin_bit_cast(f16x8, a), acc, 0, 0, 0);
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    int l = it.l0, k0 = 0;
    bool have = l < it.l1;
    SpmmTBlock b = {0, 0, 0};
    Frag16 cur = {};
    if (have) { b = p.blocks[l]; fetch(b, 0, cur); }
    while (have) {
        int nl = l, nk = k0 + kPass16;
        SpmmTBlock nb = b;
        if (nk >= b.h) {
            nl = l + 1; nk = 0;
            if (nl < it.l1) nb = p.blocks[nl];
        }
        const bool nhave = nl < it.l1;
        Frag16 nxt = {};
        if (nhave) fetch(nb, nk, nxt);
        mma(cur.x0, cur.a0, acc);
        mma(cur.x1, cur.a1, acc);
        cur = nxt; b = nb; l = nl; k0 = nk; have = nhave;
    }
    st_store(acc, p.Ct, p.ldo, col, q_ok, n0, p.n_cols, g, p.accumulate);
}

}  // namespace

void launch_spmm_t(int dtype, unsigned n_items, hipStream_t st, const SpmmTParams& p) {
    if (n_items == 0 || p.n_cols <= 0) return;
    const dim3 grid(n_items, (unsigned)((p.n_cols + kSpmmTSlab - 1) / kSpmmTSlab));
    if (dtype == SPARTA_F32) hipLaunchKernelGGL(vbs_spmm_t_f32_kernel, grid, dim3(kThreads), 0, st, p);
    else if (dtype == SPARTA_BF16) hipLaunchKernelGGL(vbs_spmm_t_h16_kernel<true>, grid, dim3(kThreads), 0, st, p);
    else hipLaunchKernelGGL(vbs_spmm_t_h16_kernel<false>, grid, dim3(kThreads), 0, st, p);
}

}  // namespace sparta_dev
