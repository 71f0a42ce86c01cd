// fl_host_tier.hpp -- the host tier of the C ABI (fl_<ty>_*_host, fl_host_release): the per-thread context, its staging buffers and the
// zero-copy completion word.  Included by exactly one translation unit of the library (fl_capi.hip), as fl_scan.hpp and
// fl_consumer_tier.hpp are: k_host_done
// below is part of that file's code object, and host_unpack_single calls its dev_unpack_single (declared here, defined there).
#pragma once
#include "fl_host.hpp"
#include "fl_kernels.hpp"

#include <atomic>
#include <chrono>
#include <cstring>

namespace {

using namespace fl;

template <typename T>
int dev_unpack_single(unsigned w, const T* packed, size_t n_blocks, const uint64_t* idx, size_t n_idx, T* out, uint32_t* err_flag, void* s);

// ---------------------------------------------------------------------------
// Host tier: the trait methods' host slices, run through the same kernels.
//
// The reference is allocation-free (`#![no_std]`, lib.rs:3); so is this tier after its first call
// on a thread: every host thread keeps ONE cached context (HostCtx, thread_local) holding
//   * a private non-blocking stream (concurrent host threads do not serialise on the null stream),
//   * a pinned, device-mapped staging buffer and a device scratch buffer, both grown geometrically
//     and freed at thread exit or by fl_host_release().
// Small calls (one trait-method call = one block) are ZERO-COPY: the slices are copied into the
// pinned buffer and the kernel reads / writes that host memory directly over PCIe -- one launch, no DMA
// round trips, completion signalled through a word in pinned memory (HostCtx::wait_zero_copy).  Large calls
// stage through the device scratch buffer.
// ---------------------------------------------------------------------------
// the last thing queued behind a zero-copy call: one thread stores the call's sequence number into pinned host memory
__global__ void k_host_done(uint64_t* flag, uint64_t seq)
{
    __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// zero-copy calls whose completion word did not arrive within the spin's bound (each cost a 50 ms stall and a real synchronise):
// fl_internal_zero_copy_fallbacks() -- a 50-ms-per-call cliff must not be silent
std::atomic<uint64_t> g_zero_copy_fallbacks{0};

struct HostCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    char* dev = nullptr;
    size_t dev_cap = 0;
    char* pin = nullptr;
    size_t pin_cap = 0;
    uint64_t* done = nullptr;      // pinned: the sequence number of the last finished zero-copy call (k_host_done)
    uint64_t seq = 0;
    unsigned since_sync = 0;

    // Best effort: runs from fl_host_release() and from the thread_local destructor, i.e. possibly while the process is
    // tearing down.  If the runtime no longer answers (hipGetDevice fails) or the context's device cannot be made current,
    // nothing is freed -- leaking at exit is harmless, calling into a torn-down runtime is not.  Long-lived worker
    // threads should call fl_host_release() themselves before they exit.
    void release()
    {
        if (device < 0) return;
        int cur = -1;
        bool usable = hipGetDevice(&cur) == hipSuccess;
        bool switched = false;
        if (usable && cur != device) usable = switched = hipSetDevice(device) == hipSuccess;
        if (usable) {
            if (stream) (void)hipStreamSynchronize(stream);
            if (stream) (void)hipStreamDestroy(stream);
            if (dev) (void)hipFree(dev);
            if (pin) (void)hipHostFree(pin);
            if (done) (void)hipHostFree(done);
            if (switched) (void)hipSetDevice(cur);
        }
        stream = nullptr; dev = nullptr; pin = nullptr; done = nullptr;
        dev_cap = pin_cap = 0;
        seq = 0; since_sync = 0;
        device = -1;
    }
    // Completion of everything queued on `stream` by a ZERO-COPY call (its results are in pinned host memory once the kernel has
    // retired).  hipStreamSynchronize costs ~9 of such a call's 13 us; a one-thread kernel queued behind the work that stores the
    // call's sequence number into pinned memory, and a host spin on that word, cost ~2.4 us less (tools/exp_host_sync.hip,
    // profiles/exp_host_sync_r04.txt: 13.1 -> 10.7 us).  The spin is bounded: if the number has not arrived after ~50 ms -- a kernel
    // that faulted never stores it -- or the marker cannot be launched, the stream is synchronised the ordinary way, which also
    // reports the error.  Every 4096th call synchronises for real so that the runtime retires its completion records.
    hipError_t wait_zero_copy()
    {
        if (!done || ++since_sync >= 4096) { since_sync = 0; return hipStreamSynchronize(stream); }
        const uint64_t want = ++seq;
        FL_LAUNCH(k_host_done, dim3(1), dim3(1), 0, stream, done, want);
        if (hipGetLastError() != hipSuccess) return hipStreamSynchronize(stream);
        std::chrono::steady_clock::time_point t0;
        for (unsigned spins = 0;; ++spins) {
            if (__atomic_load_n(done, __ATOMIC_ACQUIRE) == want) return hipSuccess;
            if ((spins & 0xffffu) == 0xffffu) {                   // every 65 536 polls (some tens of us): look at the clock
                const auto now = std::chrono::steady_clock::now();
                if (spins == 0xffffu) t0 = now;
                else if (now - t0 > std::chrono::milliseconds(50)) {                  // never seen in a healthy run: make it visible
                    g_zero_copy_fallbacks.fetch_add(1, std::memory_order_relaxed);
                    return hipStreamSynchronize(stream);
                }
            }
        }
    }
    // bind to the calling thread's current device
    hipError_t bind()
    {
        int cur = 0;
        hipError_t e = hipGetDevice(&cur);
        if (e != hipSuccess) return e;
        if (cur == device) return hipSuccess;
        release();
        e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        if (e != hipSuccess) { stream = nullptr; return e; }
        device = cur;
        // fine-grained (coherent) and mapped, explicitly: the host must SEE the marker's system-scope store without a synchronising
        // call, which hipHostMallocDefault only implies
        if (hipHostMalloc(reinterpret_cast<void**>(&done), 64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess) *done = 0;
        else { done = nullptr; (void)hipGetLastError(); }          // no marker word: wait_zero_copy() synchronises the stream instead
        seq = 0;
        return hipSuccess;
    }
    static size_t grown(size_t need, size_t have) { return need > 2 * have ? need : 2 * have; }
    hipError_t need_pinned(size_t bytes)
    {
        if (bytes <= pin_cap) return hipSuccess;
        if (pin) {
            hipError_t es = hipStreamSynchronize(stream);          // a kernel may still be using the old buffer
            if (es != hipSuccess) return es;
            (void)hipHostFree(pin); pin = nullptr; pin_cap = 0;
        }
        const size_t cap = grown(bytes, pin_cap < 65536 ? 65536 : pin_cap);
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&pin), cap, hipHostMallocCoherent | hipHostMallocMapped);   // see `done`
        if (e == hipSuccess) pin_cap = cap; else pin = nullptr;
        return e;
    }
    hipError_t need_device(size_t bytes)
    {
        if (bytes <= dev_cap) return hipSuccess;
        if (dev) {
            hipError_t es = hipStreamSynchronize(stream);
            if (es != hipSuccess) return es;
            (void)hipFree(dev); dev = nullptr; dev_cap = 0;
        }
        const size_t cap = grown(bytes, dev_cap);
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), cap);
        if (e == hipSuccess) dev_cap = cap; else dev = nullptr;
        return e;
    }
    ~HostCtx() { release(); }
};
thread_local HostCtx g_host;

constexpr size_t HOST_ZERO_COPY_LIMIT = 256 * 1024;   // bytes (in + aux + out) served straight from pinned host memory

#define FL_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return hip_fail(e_); } while (0)

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

// dev(in, aux, out, stream) launches the device-tier op on pointers the GPU can reach.
template <typename T, typename F>
int host_run(const T* in, size_t in_elems, const T* aux, size_t aux_elems, T* out, size_t out_elems, F&& dev)
{
    if ((in_elems && !in) || (out_elems && !out) || (aux_elems && !aux)) return FL_ERR_NULL;
    const size_t ib = in_elems * sizeof(T), ab = aux_elems * sizeof(T), ob = out_elems * sizeof(T);
    const size_t o_aux = pad256(ib), o_out = o_aux + pad256(ab), total = o_out + pad256(ob);
    HostCtx& c = g_host;
    FL_HIP(c.bind());
    fl::constructed_pair_this_thread() = false;             // the host tier's own staging buffers (a device-tier call may have left it set)
    if (total <= HOST_ZERO_COPY_LIMIT) {
        FL_HIP(c.need_pinned(total));
        if (ib) memcpy(c.pin, in, ib);
        if (ab) memcpy(c.pin + o_aux, aux, ab);
        int rc = dev(reinterpret_cast<const T*>(c.pin), reinterpret_cast<const T*>(c.pin + o_aux),
                     reinterpret_cast<T*>(c.pin + o_out), c.stream);
        if (rc != FL_OK) return rc;
        FL_HIP(c.wait_zero_copy());
        if (ob) memcpy(out, c.pin + o_out, ob);
        return FL_OK;
    }
    FL_HIP(c.need_device(total));
    if (ib) FL_HIP(hipMemcpyAsync(c.dev, in, ib, hipMemcpyHostToDevice, c.stream));
    if (ab) FL_HIP(hipMemcpyAsync(c.dev + o_aux, aux, ab, hipMemcpyHostToDevice, c.stream));
    int rc = dev(reinterpret_cast<const T*>(c.dev), reinterpret_cast<const T*>(c.dev + o_aux),
                 reinterpret_cast<T*>(c.dev + o_out), c.stream);
    if (rc != FL_OK) return rc;
    if (ob) FL_HIP(hipMemcpyAsync(out, c.dev + o_out, ob, hipMemcpyDeviceToHost, c.stream));
    FL_HIP(hipStreamSynchronize(c.stream));
    return FL_OK;
}

// unpack_single on host slices: only the indexed block travels (128*W bytes into the pinned buffer;
// the kernel then touches the one or two words bitpacking.rs:164-178 reads).
template <typename T>
int host_unpack_single(unsigned w, const T* pk, size_t n_blocks, uint64_t index, T* value)
{
    if (over_width<T>(w)) return FL_ERR_WIDTH;
    if (!value) return FL_ERR_NULL;
    if (w == 0) { *value = 0; return FL_OK; }                 // bitpacking.rs:136-139 precedes the assert
    if (index >= (uint64_t)n_blocks * 1024) return FL_ERR_INDEX;   // bitpacking.rs:152
    if (!pk) return FL_ERR_NULL;
    const size_t pl = (size_t)1024 * w / Elem<T>::BITS, pb = pl * sizeof(T);
    const size_t o_idx = pad256(pb), o_val = o_idx + 256;
    HostCtx& c = g_host;
    FL_HIP(c.bind());
    FL_HIP(c.need_pinned(o_val + 256));
    memcpy(c.pin, pk + (index >> 10) * pl, pb);
    *reinterpret_cast<uint64_t*>(c.pin + o_idx) = index & 1023u;
    int rc = dev_unpack_single<T>(w, reinterpret_cast<const T*>(c.pin), 1, reinterpret_cast<const uint64_t*>(c.pin + o_idx), 1,
                                  reinterpret_cast<T*>(c.pin + o_val), nullptr, c.stream);
    if (rc != FL_OK) return rc;
    FL_HIP(c.wait_zero_copy());
    *value = *reinterpret_cast<const T*>(c.pin + o_val);
    return FL_OK;
}

template <typename T> size_t plen(unsigned w) { return (size_t)1024 * w / Elem<T>::BITS; }

}  // namespace
