// k_update.hip -- sparta_vbs_set_values: new values (nztot floats in the mab layout: column-major h x w blocks back to back) written into
// the device images of a handle made with SPARTA_CREATE_UPDATABLE, without touching its plans.  Three kernels, all memory-bound:
//   vbs_update_copy_kernel      the reference-layout image of an fp32 handle (d_A is mab itself)
//   vbs_update_f32_frag_kernel  the fragment image of the fp32 one-tile plan (k_f32_direct.hip), k-compaction redone per step
//   vbs_update_h16_kernel       the 16-bit slices of the stream plans and of the hub plan (k_h16.hip, k_hub16.hip)
//   vbs_spmm_t_image_kernel     the 16-bit image of the transposed product (k_spmm_t.hip), handles made with SPARTA_CREATE_TRANSPOSE as well
// sparta_vbs_sgd_step compiles the fragment kernel and the slice kernel a second time with another VALUE SOURCE (k_update_image.inc): where set_values loads
// mab[i], vbs_sgd_f32_frag_kernel and vbs_sgd_h16_kernel load W[i], G[i] (and M[i]), do the SGD arithmetic in registers, store W[i] (and M[i]) and hand the
// new weight to the code that ballots, rounds and places it.  That is right only where the kernel's image holds every stored element exactly once
// (sgd_fused_image, vbs_capi.cpp, decides from the plan); everywhere else
//   vbs_sgd_step_kernel         the same arithmetic, elementwise over nztot floats, runs in front of the set_values launches
// sparta_vbs_adam_step is a third value source, AdamStep (W, G, M, V and the device-resident step state S): vbs_adam_f32_frag_kernel, vbs_adam_h16_kernel and the
// elementwise vbs_adam_step_kernel, behind the one-wave vbs_adam_tick_kernel that advances S once per step.
// sparta_vbs_sgd_step_ctl / sparta_vbs_adam_step_ctl reach the same kernels with a control record (k_gradctl.hip) in the value source: its coef multiplies g, its
// skip flag turns the step into sparta_vbs_set_values(A, W) -- W, M, V, S keep their bits, every image is written from W.
// LIVE STEPS (sparta_vbs_set_live_steps with a live-block set installed): k_update_image.inc is compiled once more per stepping source (vbs_sgdlive_* /
// vbs_adamlive_*) with a test in front of the value source -- a lane whose elements lie in a dead block does not call it: no load, no store, +0.0f handed on;
// the test reads one word per step / per slice half that k_live.hip derives from the snapshot.  The two-pass form walks the block
// table of k_prune.hip instead of the flat array (vbs_sgdlive_blocks_kernel / vbs_adamlive_blocks_kernel: one wave per block, a dead block costs one byte read).
// The names avoid "vbs_sgd_" / "vbs_adam_" on purpose: the tests count the plain kernels by those, as "vbs_sdlive_" avoids "sddmm" in k_sddmm.hip.
// Every kernel writes exactly the elements creation wrote (the slices behind the end of an image keep what creation left there) and reads mab
// only where the plan says a stored element is: nothing is read past mab + nztot.  Offsets are 64-bit throughout.
#include "vbs_kernel_common.hpp"

namespace sparta_dev {
namespace {

constexpr int kUpdMaxGrid = 65536;      // grid cap, as launch_f32_legacy_from_frag

// One element of torch.optim.SGD (dampening 0, no Nesterov), every operation rounded once to fp32 in the order include/sparta_amd.h pins: no contraction
// into FMAs, so a float32 restatement on the host reproduces W and M bit for bit.  m is read and written only when momentum != 0.
// ctl: the step runs under a control record (sparta_vbs_sgd_step_ctl with R != NULL), whose coef then multiplies g, whatever its value.
__device__ __forceinline__ float sgd_element(const SgdCfg& c, bool ctl, float coef, float w, float g, float& m) {
#pragma clang fp contract(off)
    if (c.grad_scale != 1.0f) g = g * c.grad_scale;
    if (ctl) g = g * coef;
    if (c.weight_decay != 0.0f) g = g + c.weight_decay * w;
    if (c.momentum != 0.0f) { m = c.momentum * m + g; g = m; }
    return w - c.lr * g;
}

// The value source of the image kernels of sparta_vbs_sgd_step.  step<N> updates the N elements i0, i0 + stride, ... of W (and M) and returns the new weights:
// ALL loads first, then the arithmetic, then the stores, so that the N (2 N, 3 N) loads of a lane are in flight together as the N loads of the set_values
// kernels are -- element by element (load, wait, store, load, ...) the image kernels ran N dependent round trips to memory per lane.
// R != nullptr: coef and skip are read from the control record at every launch (a replay reads them afresh).  Under skip the values handed on are W as it
// stands -- G, M are not even loaded, nothing is stored: the image is written from W and nothing non-finite can come near it.
struct SgdStep {
    float* __restrict__ W; const float* __restrict__ G; float* __restrict__ M;
    SgdCfg c;
    const uint32_t* __restrict__ R;
    __device__ __forceinline__ float coef() const { return R != nullptr ? __uint_as_float(R[kGradCtlCoef]) : 1.0f; }
    __device__ __forceinline__ bool skip() const { return R != nullptr && R[kGradCtlSkip] != 0u; }
    template <int N>
    __device__ __forceinline__ void step(int64_t i0, int64_t stride, float (&x)[N]) const {
        if (skip()) {
#pragma unroll
            for (int e = 0; e < N; e++) x[e] = W[i0 + e * stride];
            return;
        }
        const bool mom = c.momentum != 0.0f, ctl = R != nullptr;
        const float cf = coef();
        float w[N], g[N], m[N];
#pragma unroll
        for (int e = 0; e < N; e++) { w[e] = W[i0 + e * stride]; g[e] = G[i0 + e * stride]; m[e] = mom ? M[i0 + e * stride] : 0.0f; }
#pragma unroll
        for (int e = 0; e < N; e++) x[e] = sgd_element(c, ctl, cf, w[e], g[e], m[e]);
#pragma unroll
        for (int e = 0; e < N; e++) { W[i0 + e * stride] = x[e]; if (mom) M[i0 + e * stride] = m[e]; }
    }
};

// The two-pass form of sparta_vbs_sgd_step: W, G, M are the caller's arrays (any 4-byte boundary), 16 bytes per lane and access, the last n % 4 one by one.
// Under skip it does nothing: the set_values launches behind it write the images from the W that stands.
__global__ __launch_bounds__(kThreads) void vbs_sgd_step_kernel(int64_t n, SgdStep s) {
    if (s.skip()) return;
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * kThreads;
    const bool mom = s.c.momentum != 0.0f, ctl = s.R != nullptr;
    const float cf = s.coef();
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride) {
        f32x4 w = *reinterpret_cast<const f32x4u*>(s.W + 4 * i);
        const f32x4 g = *reinterpret_cast<const f32x4u*>(s.G + 4 * i);
        f32x4 m = {0.0f, 0.0f, 0.0f, 0.0f};
        if (mom) m = *reinterpret_cast<const f32x4u*>(s.M + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; e++) { float me = m[e]; w[e] = sgd_element(s.c, ctl, cf, w[e], g[e], me); m[e] = me; }
        if (mom) *reinterpret_cast<f32x4u*>(s.M + 4 * i) = m;
        *reinterpret_cast<f32x4u*>(s.W + 4 * i) = w;
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) { float x[1]; s.step<1>(i, 1, x); }
}

// ---- the value source of sparta_vbs_adam_step ---------------------------------------------------------------------------------------------------
// The once-per-step block of include/sparta_amd.h: the step count and the running products of the betas live in S (device memory), so that a captured step
// advances them at every replay.  Every operation rounded once to fp32; the division and the square root are the correctly rounded ones (no fast-math flag
// on this file).
__device__ __forceinline__ void adam_tick(float beta1, float beta2, float lr, int32_t& t, float& p1, float& p2, float& step_size, float& d) {
#pragma clang fp contract(off)
    if (t == 0) { p1 = beta1; p2 = beta2; } else { p1 = p1 * beta1; p2 = p2 * beta2; }
    t = t + 1;
    const float bc1 = 1.0f - p1, bc2 = 1.0f - p2;
    step_size = lr / bc1;
    d = sqrtf(bc2);
}

// One wave, one lane at work: S[0] = t, S[1], S[2] = the running products, S[3] = step_size, S[4] = d, S[5..7] = 0 (4-byte accesses: S may sit on any
// 4-byte boundary).  The element kernels behind it in the stream read S[3] and S[4].  R: the control record or nullptr; a skipped step leaves S as it is.
__global__ __launch_bounds__(64) void vbs_adam_tick_kernel(uint32_t* S, float beta1, float beta2, float lr, const uint32_t* R) {
    if (threadIdx.x != 0) return;
    if (R != nullptr && R[kGradCtlSkip] != 0u) return;
    int32_t t = (int32_t)S[0];
    float p1 = __uint_as_float(S[1]), p2 = __uint_as_float(S[2]), step_size, d;
    adam_tick(beta1, beta2, lr, t, p1, p2, step_size, d);
    S[0] = (uint32_t)t; S[1] = __float_as_uint(p1); S[2] = __float_as_uint(p2); S[3] = __float_as_uint(step_size); S[4] = __float_as_uint(d);
    S[5] = 0u; S[6] = 0u; S[7] = 0u;
}

// One element of torch.optim.AdamW (decoupled) / torch.optim.Adam with L2 weight decay (no amsgrad, no maximize) in the order include/sparta_amd.h pins, one
// rounding per operation, no contraction: a float32 restatement on the host reproduces W, M and V bit for bit.
__device__ __forceinline__ float adam_element(const AdamCfg& c, bool ctl, float coef, float step_size, float d, float w, float g, float& m, float& v) {
#pragma clang fp contract(off)
    if (c.grad_scale != 1.0f) g = g * c.grad_scale;
    if (ctl) g = g * coef;                     // (as sgd_element)
    if (c.weight_decay != 0.0f) {
        if (c.decoupled) w = w * c.dk;
        else g = g + c.weight_decay * w;
    }
    m = c.beta1 * m + c.omb1 * g;
    v = c.beta2 * v + c.omb2 * (g * g);
    const float den = sqrtf(v) / d + c.eps;
    return w - step_size * (m / den);
}

// The interface of SgdStep: all 4 N loads of a lane first, then the arithmetic, then the 3 N stores.  step_size and d are what the tick wrote for this step.
// R as in SgdStep.
struct AdamStep {
    float* __restrict__ W; const float* __restrict__ G; float* __restrict__ M; float* __restrict__ V; const float* __restrict__ S;
    AdamCfg c;
    const uint32_t* __restrict__ R;
    __device__ __forceinline__ float coef() const { return R != nullptr ? __uint_as_float(R[kGradCtlCoef]) : 1.0f; }
    __device__ __forceinline__ bool skip() const { return R != nullptr && R[kGradCtlSkip] != 0u; }
    template <int N>
    __device__ __forceinline__ void step(int64_t i0, int64_t stride, float (&x)[N]) const {
        if (skip()) {
#pragma unroll
            for (int e = 0; e < N; e++) x[e] = W[i0 + e * stride];
            return;
        }
        const bool ctl = R != nullptr;
        const float cf = coef();
        const float step_size = S[3], d = S[4];
        float w[N], g[N], m[N], v[N];
#pragma unroll
        for (int e = 0; e < N; e++) { w[e] = W[i0 + e * stride]; g[e] = G[i0 + e * stride]; m[e] = M[i0 + e * stride]; v[e] = V[i0 + e * stride]; }
#pragma unroll
        for (int e = 0; e < N; e++) x[e] = adam_element(c, ctl, cf, step_size, d, w[e], g[e], m[e], v[e]);
#pragma unroll
        for (int e = 0; e < N; e++) { W[i0 + e * stride] = x[e]; M[i0 + e * stride] = m[e]; V[i0 + e * stride] = v[e]; }
    }
};

// The two-pass form of sparta_vbs_adam_step, shaped as vbs_sgd_step_kernel: 16 bytes per lane and access, the last n % 4 one by one.
__global__ __launch_bounds__(kThreads) void vbs_adam_step_kernel(int64_t n, AdamStep s) {
    if (s.skip()) return;
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * kThreads;
    const bool ctl = s.R != nullptr;
    const float cf = s.coef();
    const float step_size = s.S[3], d = s.S[4];
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride) {
        f32x4 w = *reinterpret_cast<const f32x4u*>(s.W + 4 * i);
        const f32x4 g = *reinterpret_cast<const f32x4u*>(s.G + 4 * i);
        f32x4 m = *reinterpret_cast<const f32x4u*>(s.M + 4 * i);
        f32x4 v = *reinterpret_cast<const f32x4u*>(s.V + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; e++) { float me = m[e], ve = v[e]; w[e] = adam_element(s.c, ctl, cf, step_size, d, w[e], g[e], me, ve); m[e] = me; v[e] = ve; }
        *reinterpret_cast<f32x4u*>(s.M + 4 * i) = m;
        *reinterpret_cast<f32x4u*>(s.V + 4 * i) = v;
        *reinterpret_cast<f32x4u*>(s.W + 4 * i) = w;
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) { float x[1]; s.step<1>(i, 1, x); }
}

// ---- the two-pass form of the live steps --------------------------------------------------------------------------------------------------------
// The block table of k_prune.hip (PruneBlock: first element, n_all elements, mab order) walked as vbs_prune_mask_kernel walks it: one WAVE per block, kPruneWaves
// to a workgroup, a block never split.  A wave whose block is dead in the snapshot returns after one byte read: nothing of W, G, M, V is read or written, the
// positions past `cols` included (n_all covers them).  A live block: the elements up to the first 16-byte boundary of W one per lane, the body 16 bytes per
// lane and access (G, M, V at the same offsets: tensors of one allocator share W's alignment modulo 16; the accesses are right on any 4-byte boundary), the
// last (n - head) % 4 one per lane.  The arithmetic is sgd_element / adam_element per element: the bits of the flat kernels.
__device__ __forceinline__ int upd_head(const float* p, int n) {
    const int to_boundary = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    return n < to_boundary ? n : to_boundary;
}

__global__ __launch_bounds__(kThreads) void vbs_sgdlive_blocks_kernel(const PruneBlock* __restrict__ blocks, int64_t n_blocks, const uint8_t* __restrict__ keep, SgdStep s) {
    const int64_t b = (int64_t)blockIdx.x * kPruneWaves + (threadIdx.x >> 6);
    if (b >= n_blocks || keep[b] == 0 || s.skip()) return;      // (the whole wave)
    const int lane = threadIdx.x & 63;
    const PruneBlock blk = blocks[b];
    const int n = blk.n_all, head = upd_head(s.W + blk.off, n), n4 = (n - head) >> 2;
    const int64_t body = blk.off + head;
    const bool mom = s.c.momentum != 0.0f, ctl = s.R != nullptr;
    const float cf = s.coef();
    for (int i = lane; i < n4; i += 64) {
        f32x4 w = *reinterpret_cast<const f32x4u*>(s.W + body + 4 * i);
        const f32x4 g = *reinterpret_cast<const f32x4u*>(s.G + body + 4 * i);
        f32x4 m = {0.0f, 0.0f, 0.0f, 0.0f};
        if (mom) m = *reinterpret_cast<const f32x4u*>(s.M + body + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; e++) { float me = m[e]; w[e] = sgd_element(s.c, ctl, cf, w[e], g[e], me); m[e] = me; }
        if (mom) *reinterpret_cast<f32x4u*>(s.M + body + 4 * i) = m;
        *reinterpret_cast<f32x4u*>(s.W + body + 4 * i) = w;
    }
    float x[1];
    if (lane < head) s.step<1>(blk.off + lane, 1, x);
    const int t = head + 4 * n4 + lane;
    if (t < n) s.step<1>(blk.off + t, 1, x);
}

__global__ __launch_bounds__(kThreads) void vbs_adamlive_blocks_kernel(const PruneBlock* __restrict__ blocks, int64_t n_blocks, const uint8_t* __restrict__ keep, AdamStep s) {
    const int64_t b = (int64_t)blockIdx.x * kPruneWaves + (threadIdx.x >> 6);
    if (b >= n_blocks || keep[b] == 0 || s.skip()) return;      // (the whole wave)
    const int lane = threadIdx.x & 63;
    const PruneBlock blk = blocks[b];
    const int n = blk.n_all, head = upd_head(s.W + blk.off, n), n4 = (n - head) >> 2;
    const int64_t body = blk.off + head;
    const bool ctl = s.R != nullptr;
    const float cf = s.coef();
    const float step_size = s.S[3], d = s.S[4];
    for (int i = lane; i < n4; i += 64) {
        f32x4 w = *reinterpret_cast<const f32x4u*>(s.W + body + 4 * i);
        const f32x4 g = *reinterpret_cast<const f32x4u*>(s.G + body + 4 * i);
        f32x4 m = *reinterpret_cast<const f32x4u*>(s.M + body + 4 * i);
        f32x4 v = *reinterpret_cast<const f32x4u*>(s.V + body + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; e++) { float me = m[e], ve = v[e]; w[e] = adam_element(s.c, ctl, cf, step_size, d, w[e], g[e], me, ve); m[e] = me; v[e] = ve; }
        *reinterpret_cast<f32x4u*>(s.M + body + 4 * i) = m;
        *reinterpret_cast<f32x4u*>(s.V + body + 4 * i) = v;
        *reinterpret_cast<f32x4u*>(s.W + body + 4 * i) = w;
    }
    float x[1];
    if (lane < head) s.step<1>(blk.off + lane, 1, x);
    const int t = head + 4 * n4 + lane;
    if (t < n) s.step<1>(blk.off + t, 1, x);
}

__global__ __launch_bounds__(kThreads) void vbs_update_copy_kernel(const float* __restrict__ mab, int64_t n, float* __restrict__ A) {
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += stride)      // (the caller's array may start on any 4-byte boundary)
        *reinterpret_cast<f32x4*>(A + 4 * i) = *reinterpret_cast<const f32x4u*>(mab + 4 * i);
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) A[i] = mab[i];
}

// (upd_h16, the fp32 -> fp16 / bf16 rounding of every image, lives in vbs_kernel_common.hpp: k_epilogue.hip rounds with it too)
// the fragment kernel and the slice kernel, once per value source
#define UPD_SOURCE 0
#include "k_update_image.inc"
#undef UPD_SOURCE
#define UPD_SOURCE 1
#include "k_update_image.inc"
#undef UPD_SOURCE
#define UPD_SOURCE 2
#include "k_update_image.inc"
#undef UPD_SOURCE
// ... and the live form of the two stepping sources
#define UPD_SOURCE 1
#define UPD_LIVE 1
#include "k_update_image.inc"
#undef UPD_SOURCE
#define UPD_SOURCE 2
#define UPD_LIVE 1
#include "k_update_image.inc"
#undef UPD_SOURCE

// The image of sparta_vbs_spmm_t: per block [ceil(h / 8)][w][8] -- chunk c = kc * w + q holds rows 8 kc .. 8 kc + 7 of stored column q (rows past h: zeros), what
// pack_spmm_t_block (vbs_plan.cpp) writes at creation.  One wave per block and pass; a lane writes one 16-byte chunk from 8 consecutive floats of one column of mab.
template <bool BF16>
__global__ __launch_bounds__(kThreads) void vbs_spmm_t_image_kernel(const SpmmTSrc* __restrict__ src, int64_t n_blocks, int w, const float* __restrict__ mab, uint16_t* __restrict__ dst) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t bi = (int64_t)blockIdx.x * (kThreads / 64) + wave; bi < n_blocks; bi += (int64_t)gridDim.x * (kThreads / 64)) {
        const SpmmTSrc s = src[bi];
        const int64_t chunks = (int64_t)((s.h + 7) / 8) * w;
        for (int64_t c = lane; c < chunks; c += 64) {
            const int64_t kc = c / w, q = c - kc * w;
            const float* sp = mab + s.src + q * s.h + kc * 8;
            const int rem = s.h - (int)(kc * 8);
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; e++) x[e] = e < rem ? sp[e] : 0.0f;
            u32x4 o;
#pragma unroll
            for (int e = 0; e < 4; e++) o[e] = upd_h16<BF16>(x[2 * e]) | (upd_h16<BF16>(x[2 * e + 1]) << 16);
            *reinterpret_cast<u32x4*>(dst + s.dst + c * 8) = o;
        }
    }
}

unsigned upd_grid(int64_t work_items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(work_items, kUpdMaxGrid)); }

template <bool BF16>
void launch_update_h16_t(bool hub, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const float* mab, uint16_t* dst) {
    const dim3 block(kThreads);
    if (hub) hipLaunchKernelGGL((vbs_update_h16_kernel<BF16, true, 64, 64>), dim3(upd_grid(n_slices * 2)), block, 0, st, map, n_slices, mab, dst);
    else if (tms == 32 && kp == 32) hipLaunchKernelGGL((vbs_update_h16_kernel<BF16, false, 32, 32>), dim3(upd_grid((n_slices + 1) / 2)), block, 0, st, map, n_slices, mab, dst);
    else if (tms == 64 && kp == 32) hipLaunchKernelGGL((vbs_update_h16_kernel<BF16, false, 64, 32>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, mab, dst);
    else if (tms == 32 && kp == 64) hipLaunchKernelGGL((vbs_update_h16_kernel<BF16, false, 32, 64>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, mab, dst);
    else hipLaunchKernelGGL((vbs_update_h16_kernel<BF16, false, 64, 64>), dim3(upd_grid(n_slices * 2)), block, 0, st, map, n_slices, mab, dst);
}

template <bool BF16>
void launch_sgd_h16_t(int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const SgdStep& vs, uint16_t* dst) {     // the grids of launch_update_h16_t
    const dim3 block(kThreads);
    if (tms == 32 && kp == 32) hipLaunchKernelGGL((vbs_sgd_h16_kernel<BF16, 32, 32>), dim3(upd_grid((n_slices + 1) / 2)), block, 0, st, map, n_slices, vs, dst);
    else if (tms == 64 && kp == 32) hipLaunchKernelGGL((vbs_sgd_h16_kernel<BF16, 64, 32>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, vs, dst);
    else if (tms == 32 && kp == 64) hipLaunchKernelGGL((vbs_sgd_h16_kernel<BF16, 32, 64>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, vs, dst);
    else hipLaunchKernelGGL((vbs_sgd_h16_kernel<BF16, 64, 64>), dim3(upd_grid(n_slices * 2)), block, 0, st, map, n_slices, vs, dst);
}

template <bool BF16>
void launch_adam_h16_t(int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const AdamStep& vs, uint16_t* dst) {   // the grids of launch_update_h16_t
    const dim3 block(kThreads);
    if (tms == 32 && kp == 32) hipLaunchKernelGGL((vbs_adam_h16_kernel<BF16, 32, 32>), dim3(upd_grid((n_slices + 1) / 2)), block, 0, st, map, n_slices, vs, dst);
    else if (tms == 64 && kp == 32) hipLaunchKernelGGL((vbs_adam_h16_kernel<BF16, 64, 32>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, vs, dst);
    else if (tms == 32 && kp == 64) hipLaunchKernelGGL((vbs_adam_h16_kernel<BF16, 32, 64>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, vs, dst);
    else hipLaunchKernelGGL((vbs_adam_h16_kernel<BF16, 64, 64>), dim3(upd_grid(n_slices * 2)), block, 0, st, map, n_slices, vs, dst);
}

template <bool BF16>
void launch_sgd_h16_live_t(int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const SgdStep& vs, uint16_t* dst, const uint32_t* words) {   // the grids of launch_update_h16_t
    const dim3 block(kThreads);
    if (tms == 32 && kp == 32) hipLaunchKernelGGL((vbs_sgdlive_h16_kernel<BF16, 32, 32>), dim3(upd_grid((n_slices + 1) / 2)), block, 0, st, map, n_slices, vs, dst, words);
    else if (tms == 64 && kp == 32) hipLaunchKernelGGL((vbs_sgdlive_h16_kernel<BF16, 64, 32>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, vs, dst, words);
    else if (tms == 32 && kp == 64) hipLaunchKernelGGL((vbs_sgdlive_h16_kernel<BF16, 32, 64>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, vs, dst, words);
    else hipLaunchKernelGGL((vbs_sgdlive_h16_kernel<BF16, 64, 64>), dim3(upd_grid(n_slices * 2)), block, 0, st, map, n_slices, vs, dst, words);
}

template <bool BF16>
void launch_adam_h16_live_t(int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const AdamStep& vs, uint16_t* dst, const uint32_t* words) {
    const dim3 block(kThreads);
    if (tms == 32 && kp == 32) hipLaunchKernelGGL((vbs_adamlive_h16_kernel<BF16, 32, 32>), dim3(upd_grid((n_slices + 1) / 2)), block, 0, st, map, n_slices, vs, dst, words);
    else if (tms == 64 && kp == 32) hipLaunchKernelGGL((vbs_adamlive_h16_kernel<BF16, 64, 32>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, vs, dst, words);
    else if (tms == 32 && kp == 64) hipLaunchKernelGGL((vbs_adamlive_h16_kernel<BF16, 32, 64>), dim3(upd_grid(n_slices)), block, 0, st, map, n_slices, vs, dst, words);
    else hipLaunchKernelGGL((vbs_adamlive_h16_kernel<BF16, 64, 64>), dim3(upd_grid(n_slices * 2)), block, 0, st, map, n_slices, vs, dst, words);
}

SgdStep sgd_source(float* W, const float* G, float* M, const SgdCfg& cfg, const uint32_t* R) { return SgdStep{W, G, cfg.momentum != 0.0f ? M : nullptr, cfg, R}; }
unsigned blocks_grid(int64_t n_blocks) { return (unsigned)((n_blocks + kPruneWaves - 1) / kPruneWaves); }

}  // namespace

void launch_update_copy(hipStream_t st, const float* mab, int64_t n, float* A) {
    if (n <= 0) return;
    hipLaunchKernelGGL(vbs_update_copy_kernel, dim3(upd_grid((n / 4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, mab, n, A);
}

void launch_update_f32_frag(hipStream_t st, StepRec* steps, int64_t n_steps, const float* mab, float* a_frag, float* A_out) {
    if (n_steps <= 0) return;
    hipLaunchKernelGGL(vbs_update_f32_frag_kernel, dim3(upd_grid((n_steps + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, st, steps, n_steps, mab, a_frag, A_out);
}

void launch_update_h16(bool bf16, bool hub, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const float* mab, uint16_t* dst) {
    if (n_slices <= 0) return;
    if (bf16) launch_update_h16_t<true>(hub, tms, kp, st, map, n_slices, mab, dst);
    else launch_update_h16_t<false>(hub, tms, kp, st, map, n_slices, mab, dst);
}

void launch_update_h16_t(bool bf16, hipStream_t st, const SpmmTSrc* src, int64_t n_blocks, int w, const float* mab, uint16_t* dst) {
    if (n_blocks <= 0) return;
    const dim3 grid(upd_grid((n_blocks + kThreads / 64 - 1) / (kThreads / 64))), block(kThreads);
    if (bf16) hipLaunchKernelGGL(vbs_spmm_t_image_kernel<true>, grid, block, 0, st, src, n_blocks, w, mab, dst);
    else hipLaunchKernelGGL(vbs_spmm_t_image_kernel<false>, grid, block, 0, st, src, n_blocks, w, mab, dst);
}


// ---- sparta_vbs_sgd_step ------------------------------------------------------------------------------------------------------------------
void launch_sgd_step(hipStream_t st, int64_t n, float* W, const float* G, float* M, const SgdCfg& cfg, const uint32_t* R) {
    if (n <= 0) return;
    hipLaunchKernelGGL(vbs_sgd_step_kernel, dim3(upd_grid((n / 4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, n, sgd_source(W, G, M, cfg, R));
}

void launch_sgd_f32_frag(hipStream_t st, StepRec* steps, int64_t n_steps, float* W, const float* G, float* M, const SgdCfg& cfg, const uint32_t* R, float* a_frag, float* A_out) {
    if (n_steps <= 0) return;
    hipLaunchKernelGGL(vbs_sgd_f32_frag_kernel, dim3(upd_grid((n_steps + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, st, steps, n_steps,
                       sgd_source(W, G, M, cfg, R), a_frag, A_out);
}

void launch_sgd_h16(bool bf16, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, float* W, const float* G, float* M, const SgdCfg& cfg, const uint32_t* R, uint16_t* dst) {
    if (n_slices <= 0) return;
    if (bf16) launch_sgd_h16_t<true>(tms, kp, st, map, n_slices, sgd_source(W, G, M, cfg, R), dst);
    else launch_sgd_h16_t<false>(tms, kp, st, map, n_slices, sgd_source(W, G, M, cfg, R), dst);
}


// ---- sparta_vbs_adam_step -----------------------------------------------------------------------------------------------------------------
void launch_adam_tick(hipStream_t st, const AdamArgs& a) {
    hipLaunchKernelGGL(vbs_adam_tick_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<uint32_t*>(a.S), a.c.beta1, a.c.beta2, a.c.lr, a.R);
}

void launch_adam_step(hipStream_t st, int64_t n, const AdamArgs& a) {
    if (n <= 0) return;
    hipLaunchKernelGGL(vbs_adam_step_kernel, dim3(upd_grid((n / 4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, n, AdamStep{a.W, a.G, a.M, a.V, a.S, a.c, a.R});
}

void launch_adam_f32_frag(hipStream_t st, StepRec* steps, int64_t n_steps, const AdamArgs& a, float* a_frag, float* A_out) {
    if (n_steps <= 0) return;
    hipLaunchKernelGGL(vbs_adam_f32_frag_kernel, dim3(upd_grid((n_steps + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, st, steps, n_steps,
                       AdamStep{a.W, a.G, a.M, a.V, a.S, a.c, a.R}, a_frag, A_out);
}

void launch_adam_h16(bool bf16, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const AdamArgs& a, uint16_t* dst) {
    if (n_slices <= 0) return;
    const AdamStep vs{a.W, a.G, a.M, a.V, a.S, a.c, a.R};
    if (bf16) launch_adam_h16_t<true>(tms, kp, st, map, n_slices, vs, dst);
    else launch_adam_h16_t<false>(tms, kp, st, map, n_slices, vs, dst);
}


// ---- the live forms (sparta_vbs_set_live_steps) -------------------------------------------------------------------------------------------
void launch_sgd_blocks_live(hipStream_t st, const PruneBlock* blocks, int64_t n_blocks, const uint8_t* keep, float* W, const float* G, float* M, const SgdCfg& cfg,
                            const uint32_t* R) {
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(vbs_sgdlive_blocks_kernel, dim3(blocks_grid(n_blocks)), dim3(kThreads), 0, st, blocks, n_blocks, keep, sgd_source(W, G, M, cfg, R));
}

void launch_sgd_f32_frag_live(hipStream_t st, StepRec* steps, int64_t n_steps, float* W, const float* G, float* M, const SgdCfg& cfg, const uint32_t* R, float* a_frag,
                              float* A_out, const uint32_t* words) {
    if (n_steps <= 0) return;
    hipLaunchKernelGGL(vbs_sgdlive_f32_frag_kernel, dim3(upd_grid((n_steps + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, st, steps, n_steps,
                       sgd_source(W, G, M, cfg, R), a_frag, A_out, words);
}

void launch_sgd_h16_live(bool bf16, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, float* W, const float* G, float* M, const SgdCfg& cfg,
                         const uint32_t* R, uint16_t* dst, const uint32_t* words) {
    if (n_slices <= 0) return;
    if (bf16) launch_sgd_h16_live_t<true>(tms, kp, st, map, n_slices, sgd_source(W, G, M, cfg, R), dst, words);
    else launch_sgd_h16_live_t<false>(tms, kp, st, map, n_slices, sgd_source(W, G, M, cfg, R), dst, words);
}

void launch_adam_blocks_live(hipStream_t st, const PruneBlock* blocks, int64_t n_blocks, const uint8_t* keep, const AdamArgs& a) {
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(vbs_adamlive_blocks_kernel, dim3(blocks_grid(n_blocks)), dim3(kThreads), 0, st, blocks, n_blocks, keep, AdamStep{a.W, a.G, a.M, a.V, a.S, a.c, a.R});
}

void launch_adam_f32_frag_live(hipStream_t st, StepRec* steps, int64_t n_steps, const AdamArgs& a, float* a_frag, float* A_out, const uint32_t* words) {
    if (n_steps <= 0) return;
    hipLaunchKernelGGL(vbs_adamlive_f32_frag_kernel, dim3(upd_grid((n_steps + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, st, steps, n_steps,
                       AdamStep{a.W, a.G, a.M, a.V, a.S, a.c, a.R}, a_frag, A_out, words);
}

void launch_adam_h16_live(bool bf16, int tms, int kp, hipStream_t st, const UpdSlice* map, int64_t n_slices, const AdamArgs& a, uint16_t* dst, const uint32_t* words) {
    if (n_slices <= 0) return;
    const AdamStep vs{a.W, a.G, a.M, a.V, a.S, a.c, a.R};
    if (bf16) launch_adam_h16_live_t<true>(tms, kp, st, map, n_slices, vs, dst, words);
    else launch_adam_h16_live_t<false>(tms, kp, st, map, n_slices, vs, dst, words);
}

}  // namespace sparta_dev
