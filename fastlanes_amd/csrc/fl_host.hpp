// fl_host.hpp -- host-side helpers shared by the C ABI's two translation units: fl_capi.hip (the codec boundary, with the host tier of
// fl_host_tier.hpp, the scans of fl_scan.hpp and the consumers of a packed column of fl_consumer_tier.hpp) and fl_pair.hip
// (fl_column_pair_alloc / _free and what stands behind them).  No kernels.  FL_DEVICE_TIER also needs fl_kernels.hpp, which both include.
#pragma once
#include "../../include/fastlanes_amd.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

namespace fl {

inline thread_local int g_last_hip_error = 0;              // fl_last_hip_error()

inline int hip_fail(hipError_t e)
{
    g_last_hip_error = (int)e;
    return FL_ERR_HIP;
}
inline int hip_status(hipError_t e) { return e == hipSuccess ? FL_OK : hip_fail(e); }

inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
// the argument checks every tier words the same way; what a failure means (FL_ERR_WIDTH, FL_ERR_INDEX, a length of 0) is the caller's
inline bool valid_type_bits(unsigned type_bits) { return type_bits == 8 || type_bits == 16 || type_bits == 32 || type_bits == 64; }
template <typename T> bool over_width(unsigned w) { return w > sizeof(T) * 8; }

// *ms = the median of `timed` runs of launch() (a status) on `s`, each between two events, after `untimed` runs; synchronous
template <typename F> int median_ms(hipStream_t s, int untimed, int timed, F&& launch, float* ms)
{
    hipEvent_t t0 = nullptr, t1 = nullptr;
    hipError_t e = hipEventCreate(&t0);
    if (e == hipSuccess) e = hipEventCreate(&t1);
    int rc = FL_OK;
    float t[8] = {0.f};
    for (int i = -untimed; i < timed && e == hipSuccess && rc == FL_OK; ++i) {
        e = hipEventRecord(t0, s);
        if (e == hipSuccess) rc = launch();
        if (e == hipSuccess && rc == FL_OK) e = hipEventRecord(t1, s);
        if (e == hipSuccess && rc == FL_OK) e = hipEventSynchronize(t1);
        if (e == hipSuccess && rc == FL_OK && i >= 0) e = hipEventElapsedTime(&t[i], t0, t1);
    }
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    if (e != hipSuccess) return hip_fail(e);
    if (rc != FL_OK) return rc;
    std::sort(t, t + timed);
    *ms = t[timed / 2];
    return FL_OK;
}

// at least two of a call's pointers inside one live FL_LAYOUT_INTERLEAVED pair (fl_pair.hip)
bool fl_in_constructed_pair(std::initializer_list<const void*> ptrs);

// FL_CHECK_DEVICE=1 (fastlanes_amd.h "Threading and device selection"): before a device-tier launch, every pointer must be
// memory the calling thread's CURRENT device can use -- its own HBM, managed memory, or pinned host memory -- and `stream` a
// stream of that device; FL_ERR_DEVICE otherwise.  Off by default (one relaxed load per call): a raw kernel launch does not
// check either, and hipPointerGetAttributes costs microseconds.
inline bool device_check_enabled()
{
    static const bool on = [] { const char* e = getenv("FL_CHECK_DEVICE"); return e && e[0] && strcmp(e, "0") != 0; }();
    return on;
}
inline int device_check(void* stream, std::initializer_list<const void*> ptrs)
{
    if (!device_check_enabled()) return FL_OK;
    int cur = -1;
    if (hipError_t e = hipGetDevice(&cur); e != hipSuccess) return hip_fail(e);
    if (stream) {
        int sdev = -1;
        if (hipStreamGetDevice(static_cast<hipStream_t>(stream), &sdev) != hipSuccess) { (void)hipGetLastError(); return FL_ERR_DEVICE; }
        if (sdev != cur) return FL_ERR_DEVICE;
    }
    for (const void* p : ptrs) {
        if (!p) continue;                                   // NULL is judged (FL_ERR_NULL or allowed) by the entry point itself
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return FL_ERR_DEVICE; }   // plain host memory
        const bool device_mem = at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeArray;
        if (device_mem && at.type != hipMemoryTypeManaged && at.device != cur) return FL_ERR_DEVICE;
        if (!device_mem && at.type != hipMemoryTypeHost) return FL_ERR_DEVICE;   // unregistered host memory
    }
    return FL_OK;
}

}  // namespace fl

// (every device-tier entry also tells the launchers whether its buffers lie inside one live FL_LAYOUT_INTERLEAVED pair: fl_kernels.hpp,
// constructed_pair_this_thread -- one relaxed load while no such pair exists)
#define FL_DEVICE_TIER(stream, ...) do { if (const int rc_ = fl::device_check(stream, {__VA_ARGS__})) return rc_; \
                                         fl::constructed_pair_this_thread() = fl::fl_in_constructed_pair({__VA_ARGS__}); } while (0)
