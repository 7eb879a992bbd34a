// vbs_epilogue.cpp -- the epilogue of a linear layer, handle-free: sparta_epilogue_fwd (Y = act(Z + bias) in the output type), sparta_epilogue_bwd
// (dZ = dY * act'(Z + bias) and the bias gradient) and sparta_epilogue_scratch_bytes.  Host code only: the operand checks (ep_check) and the tiling (ep_plan).
// Kernels: k_epilogue.hip.
// From vbs_host.hpp: SPARTA_GUARD_BEGIN / _END, DeviceCall / device_call.
#include "vbs_host.hpp"

using namespace sparta_dev;

// ---- sparta_epilogue_fwd / sparta_epilogue_scratch_bytes / sparta_epilogue_bwd (k_epilogue.hip) ----------------------------------------------------
static_assert(SPARTA_EPILOGUE_RUN == kEpRun && SPARTA_ACT_NONE == kEpNone && SPARTA_ACT_RELU == kEpRelu && SPARTA_ACT_GELU == kEpGelu,
              "include/sparta_amd.h and vbs_device.hpp disagree on the epilogue");

namespace {

struct EpOperand { const char* name; const void* ptr; int64_t ld; int32_t dtype; bool required; };

bool ep_dtype_ok(int32_t t) { return t == SPARTA_F32 || t == SPARTA_F16 || t == SPARTA_BF16; }
int64_t ep_esize(int32_t t) { return t == SPARTA_F32 ? 4 : 2; }

// what both entries refuse, in one order: sizes, act, types, leading dimensions, then -- only where there is something to do -- NULL and misaligned pointers
int ep_check(const char* entry, int64_t rows, int64_t n_cols, int32_t act, const EpOperand* ops, int n_ops, const float* bias) {
    using sparta::fail;
    const std::string e(entry);
    if (rows < 0 || n_cols < 0) return fail(SPARTA_ERR_INVALID, e + ": rows < 0 or n_cols < 0");
    if (act != SPARTA_ACT_NONE && act != SPARTA_ACT_RELU && act != SPARTA_ACT_GELU) return fail(SPARTA_ERR_INVALID, e + ": unknown act " + std::to_string(act));
    for (int i = 0; i < n_ops; i++)
        if (!ep_dtype_ok(ops[i].dtype)) return fail(SPARTA_ERR_INVALID, e + ": unknown dtype " + std::to_string(ops[i].dtype) + " of " + ops[i].name);
    for (int i = 0; i < n_ops; i++)
        if ((ops[i].ptr || ops[i].required) && ops[i].ld < rows) return fail(SPARTA_ERR_INVALID, e + ": the leading dimension of " + ops[i].name + " is below rows (ld < rows)");
    for (int i = 0; i < n_ops; i++) {
        if (!ops[i].ptr && ops[i].required && rows > 0 && n_cols > 0) return fail(SPARTA_ERR_INVALID, e + ": " + ops[i].name + " is NULL");
        if ((uintptr_t)ops[i].ptr % (uintptr_t)ep_esize(ops[i].dtype) != 0) return fail(SPARTA_ERR_INVALID, e + ": " + ops[i].name + " is not aligned to its element size");
    }
    if ((uintptr_t)bias % 4 != 0) return fail(SPARTA_ERR_INVALID, e + ": bias is not aligned to its element size");
    if (n_cols > 0 && (rows > INT64_MAX / 16 / n_cols)) return fail(SPARTA_ERR_UNSUPPORTED, e + ": rows * n_cols too large");
    for (int i = 0; i < n_ops; i++)
        if (ops[i].ptr && n_cols > 0 && ops[i].ld > INT64_MAX / 16 / n_cols) return fail(SPARTA_ERR_UNSUPPORTED, e + ": ld * n_cols too large");
    return SPARTA_OK;
}

// Where a lane may own four consecutive rows with one aligned access per operand (16 bytes of fp32, 8 bytes of a 16-bit type): every operand in use starts
// a group of four ELEMENTS at row `head` of column 0 -- the bases agree on head modulo 4 elements -- and every leading dimension is a multiple of 4, so the
// same holds in every column.  Otherwise head = n4 = 0 and every row goes through the edge tiles.  A function of the addresses modulo 16, ld modulo 4, rows
// and n_cols alone; the results do not depend on it (an element's arithmetic is the same in both kinds of tile, and the sums are per row).
void ep_plan(EpilogueParams& p, const EpOperand* ops, int n_ops) {
    int64_t head = -1;
    bool ok = true;
    for (int i = 0; i < n_ops && ok; i++) {
        if (!ops[i].ptr) continue;
        const int64_t first = (int64_t)((uintptr_t)ops[i].ptr / (uintptr_t)ep_esize(ops[i].dtype)), h = (4 - first % 4) % 4;
        if (head < 0) head = h;
        ok = h == head && (ops[i].ld % 4 == 0 || p.n_cols <= 1);
    }
    if (!ok || head < 0 || p.rows - head < 4) head = 0, p.n4 = 0;
    else p.n4 = (p.rows - head) / 4;
    p.head = head;
    p.vec_tiles = (p.n4 + 63) / 64;
    p.edge_tiles = (p.rows - 4 * p.n4 + kThreads - 1) / kThreads;
    p.n_runs = (p.n_cols + kEpRun - 1) / kEpRun;
}

int64_t ep_scratch_bytes(int64_t rows, int64_t n_cols) {
    const int64_t n_runs = (n_cols + kEpRun - 1) / kEpRun;
    return n_runs > 1 ? n_runs * rows * (int64_t)sizeof(double) : 0;
}

// the launches of one entry between two events of this call (handle-free, as sparta_grad_stats)
template <class Launch>
int ep_call(const char* entry, bool nothing_to_do, void* stream, float* dt_ms, Launch launch) {
    return device_call(DeviceCall{entry, nullptr, (hipStream_t)stream, true, dt_ms, "the kernels", nullptr, nullptr, nothing_to_do}, launch);
}

}  // namespace

extern "C" int sparta_epilogue_fwd(const float* Z, int64_t ldz, const float* bias, int32_t act, void* Y, int64_t ldy, int32_t y_dtype, int64_t rows, int64_t n_cols,
                                   void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    const EpOperand ops[2] = {{"Z", Z, ldz, SPARTA_F32, true}, {"Y", Y, ldy, y_dtype, true}};
    if (int rc = ep_check("sparta_epilogue_fwd", rows, n_cols, act, ops, 2, bias)) return rc;
    EpilogueParams p{};
    p.Z = Z; p.bias = bias; p.Out = Y; p.ldz = ldz; p.ldo = ldy; p.rows = rows; p.n_cols = n_cols; p.act = act;
    ep_plan(p, ops, 2);
    return ep_call("sparta_epilogue_fwd", rows == 0 || n_cols == 0, stream, dt_ms, [&](hipStream_t st) { launch_epilogue_fwd(st, y_dtype, p); });
    SPARTA_GUARD_END("sparta_epilogue_fwd")
}

extern "C" int sparta_epilogue_scratch_bytes(int64_t rows, int64_t n_cols, int64_t* bytes_out) {
    using sparta::fail;
    if (!bytes_out) return fail(SPARTA_ERR_INVALID, "sparta_epilogue_scratch_bytes: bytes_out is NULL");
    if (rows < 0 || n_cols < 0) return fail(SPARTA_ERR_INVALID, "sparta_epilogue_scratch_bytes: rows < 0 or n_cols < 0");
    if (n_cols > 0 && rows > INT64_MAX / 16 / n_cols) return fail(SPARTA_ERR_UNSUPPORTED, "sparta_epilogue_scratch_bytes: rows * n_cols too large");
    *bytes_out = ep_scratch_bytes(rows, n_cols);
    return SPARTA_OK;
}

extern "C" int sparta_epilogue_bwd(const void* dY, int64_t lddy, int32_t dy_dtype, const float* Z, int64_t ldz, const float* bias, int32_t act, void* dZ, int64_t lddz,
                                   int32_t dz_dtype, float* dbias, void* scratch, int64_t rows, int64_t n_cols, void* stream, float* dt_ms) {
    SPARTA_GUARD_BEGIN
    using sparta::fail;
    const EpOperand ops[3] = {{"dY", dY, lddy, dy_dtype, true}, {"Z", Z, ldz, SPARTA_F32, act != SPARTA_ACT_NONE}, {"dZ", dZ, lddz, dz_dtype, true}};
    if (int rc = ep_check("sparta_epilogue_bwd", rows, n_cols, act, ops, 3, bias)) return rc;
    if ((uintptr_t)dbias % 4 != 0) return fail(SPARTA_ERR_INVALID, "sparta_epilogue_bwd: dbias is not aligned to its element size");
    const bool partials = dbias && rows > 0 && ep_scratch_bytes(rows, n_cols) > 0;
    if (partials && !scratch) return fail(SPARTA_ERR_INVALID, "sparta_epilogue_bwd: scratch is NULL (sparta_epilogue_scratch_bytes > 0 and dbias != NULL)");
    if (partials && (uintptr_t)scratch % 8 != 0) return fail(SPARTA_ERR_INVALID, "sparta_epilogue_bwd: scratch is not aligned to 8 bytes");
    EpilogueParams p{};
    p.dY = dY; p.Z = act != SPARTA_ACT_NONE ? Z : nullptr; p.bias = act != SPARTA_ACT_NONE ? bias : nullptr; p.Out = dZ; p.dbias = dbias;
    p.part = partials ? (double*)scratch : nullptr;
    p.lddy = lddy; p.ldz = ldz; p.ldo = lddz; p.rows = rows; p.n_cols = n_cols; p.act = act;
    const EpOperand used[3] = {ops[0], {"Z", p.Z, ldz, SPARTA_F32, false}, ops[2]};      // (with act == NONE neither Z nor bias is read: u is not needed)
    ep_plan(p, used, 3);
    const bool nothing = rows == 0 || (n_cols == 0 && !dbias);                           // (n_cols == 0 with dbias: the fold kernel stores +0.0f)
    return ep_call("sparta_epilogue_bwd", nothing, stream, dt_ms, [&](hipStream_t st) { launch_epilogue_bwd(st, dy_dtype, dz_dtype, p); });
    SPARTA_GUARD_END("sparta_epilogue_bwd")
}
