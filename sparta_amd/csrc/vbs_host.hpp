// vbs_host.hpp -- what the host files of the sparta_vbs_* entry points share: the .cpp files that include it (VBS_HOST_SRCS in the Makefile).  Never included
// by a kernel file: a change here rebuilds no kernel.
// The rule: what two of those files use is here -- the exception guard and the scaffold of a device call as definitions (two macros, two structs, three
// templates), every other helper as a declaration in namespace sparta_dev with its one definition in the file named next to it.  What one file uses stays
// in that file's anonymous namespace.  No state lives here (g_capturing is in vbs_device.hpp).
#pragma once
#include <memory>
#include <optional>

#include <cmath>
#include "vbs_kernel_common.hpp"

// No exception leaves these files: the plan builder and the image builders grow large std::vectors (step lists, packed 16-bit A,
// sparse rows), so std::bad_alloc is a real outcome on 10^8..10^9-nonzero inputs and must come back as a status code.
#define SPARTA_GUARD_BEGIN try {
#define SPARTA_GUARD_END(name_)                                                                                       \
    }                                                                                                                  \
    catch (const std::bad_alloc&) { return sparta::fail(SPARTA_ERR_ALLOC, std::string(name_) + ": out of host memory"); } \
    catch (const std::exception& e) { return sparta::fail(SPARTA_ERR_INVALID, std::string(name_) + ": " + e.what()); }  \
    catch (...) { return sparta::fail(SPARTA_ERR_INVALID, std::string(name_) + ": unknown C++ exception"); }

namespace sparta_dev {

// CaptureScope sets g_capturing (vbs_device.hpp) for the duration of a call whose stream is being captured into a graph: anything that allocates,
// synchronises or times (scratch growth, the first-call autotune, the gathered step lists) then fails with SPARTA_ERR_UNSUPPORTED instead of breaking the
// capture -- run the same call once outside the capture first (same n_cols, layouts and shard_rows), after which the call is launches only.
// done(rc) is the way out of a call on a handle: a call that ran under capture and returns SPARTA_OK marks the handle as captured, after which its scratch
// is retired instead of freed when it grows (Retired, vbs_device.hpp) -- the graph holds the addresses this call launched with.
struct CaptureScope {
    explicit CaptureScope(hipStream_t st, bool device_ptrs, sparta_vbs* handle = nullptr) : handle_(handle) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        g_capturing = device_ptrs && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    }
    ~CaptureScope() { g_capturing = false; }
    int done(int rc) const {
        if (g_capturing && rc == SPARTA_OK && handle_) handle_->retired.captured = true;
        return rc;
    }
private:
    sparta_vbs* handle_;
};

// ---- the scaffold of a device entry point, in one place: DeviceGuard, CaptureScope, the refusal of a captured call that asks for dt_ms, then ev0, the
// launches, hipGetLastError, ev1 + synchronise + elapsed ----
struct DeviceCall {
    const char* entry;                          // the name the messages carry
    sparta_vbs* handle;                         // the handle whose device is made current and that a captured call marks; NULL: a handle-free entry (no guard)
    hipStream_t st;
    bool device_ptrs;                           // false: host operands -- the call synchronises anyway and CaptureScope does not look at the stream
    float* dt_ms = nullptr;                     // NULL: not timed
    const char* timed_what = nullptr;           // "the step", "the product", ...: what a captured call is refused to time (NULL: the body refuses capture itself)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;    // the handle's events; NULL: events made for this call (which synchronises anyway)
    bool nothing_to_do = false;                 // no launches: the events only
};
// what dt_ms measures: launches(st) between the two events.  Staging of host operands and ensure_* calls stay in front of it, copies back behind it.
template <class Launches>
int timed_launches(const DeviceCall& c, Launches launches) {
    DevEvent own0, own1;
    hipEvent_t e0 = c.ev0, e1 = c.ev1;
    if (c.dt_ms && !e0) {
        HIP_TRY(own0.create());
        HIP_TRY(own1.create());
        e0 = own0; e1 = own1;
    }
    if (c.dt_ms) HIP_TRY(hipEventRecord(e0, c.st));
    if (!c.nothing_to_do) {
        launches(c.st);
        HIP_TRY(hipGetLastError());
    }
    if (c.dt_ms) {
        HIP_TRY(hipEventRecord(e1, c.st));
        HIP_TRY(hipEventSynchronize(e1));
        HIP_TRY(hipEventElapsedTime(c.dt_ms, e0, e1));
    }
    return SPARTA_OK;
}
// guard, scope and refusal around body(st): a body that stages, builds lazily or reads back calls timed_launches itself (or launches untimed)
template <class Body>
int open_call(const DeviceCall& c, Body body) {
    std::optional<DeviceGuard> guard;
    if (c.handle) {
        guard.emplace(c.handle->device);
        if (!guard->ok) return sparta::fail(SPARTA_ERR_HIP, std::string(c.entry) + ": hipSetDevice failed");
    }
    const CaptureScope capture(c.st, c.device_ptrs, c.handle);
    if (g_capturing && c.dt_ms && c.timed_what) return capture_refusal((std::string("time ") + c.timed_what + " (dt_ms != NULL synchronises)").c_str(), c.entry);
    return capture.done(body(c.st));
}
// an entry that is launches only
template <class Launches>
int device_call(const DeviceCall& c, Launches launches) {
    return open_call(c, [&](hipStream_t) { return timed_launches(c, launches); });
}

// ---- helpers that cross a file boundary: one definition each, in the file named, where the comment on what it does is ----
// vbs_capi.cpp: host builders that sparta_sparse_rows_host_check / sparta_colres_host_check (vbs_host_check.cpp) run as creation runs them
int order_sparse_rows(SparseRowsHost& S, int64_t cols);
bool build_colres(int64_t rows, int64_t cols, const std::vector<int64_t>& rowptr, const std::vector<int32_t>& col, const std::vector<float>& val,
                  const std::vector<int32_t>& crow, ColresHost& H, int force_parts = 0);

}  // namespace sparta_dev
