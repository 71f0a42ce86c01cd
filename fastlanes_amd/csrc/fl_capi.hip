// fl_capi.hip -- the extern "C" boundary declared in include/fastlanes_amd.h.
// Validates arguments, maps the runtime width to the per-(T,W) kernel instance
// (the reference's `match width`, bitpacking.rs:82-95) and launches it.  No CPU
// compute path exists in this library: every entry point ends in a HIP launch.
// fl_column_pair_alloc / _free and the memory-class probe live in fl_pair.hip.
#include "../../include/fastlanes_amd.h"
#include "../../include/fastlanes_amd_internal.h"
#include "fl_host.hpp"
#include "fl_kernels.hpp"
#include "fl_misc.hpp"
#include "fl_widths.hpp"
#include "fl_chain.hpp"
#include "fl_stream.hpp"
#include "fl_batch.hpp"
#include "fl_scan.hpp"
#include "fl_consume.hpp"
#include "fl_for_compare.hpp"
#include "fl_for_compare_range.hpp"
#include "fl_select.hpp"
#include "fl_aggregate.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <new>

namespace {

using namespace fl;

// fl_internal_set_kernel_policy (validated there).  mode 0 = the generated table (fl_dispatch.hpp), 1 = cell-column kernels wherever
// they are built, 2 = wave-per-block kernels wherever they exist.  Under mode 2 the A/B tools may also force waves per SIMD (policy
// 2 + 256 * waves) and blocks per wavefront (+ 65536 * bpw, + 2^24: prefetch); bits 25-29 are the tile-map window (window_override).
// Results are bit-identical; only speed differs.
std::atomic<int> g_kernel_policy{0};
struct KernelPolicy {
    int mode;
    int waves;            // 0 = the launch's own
    unsigned bpw;         // 0 = the launch's own blocks per wavefront and prefetch
    unsigned prefetch;
};
inline KernelPolicy kernel_policy()
{
    const int p = g_kernel_policy.load(std::memory_order_relaxed);
    const bool ab = (p & 0xff) == 2;
    return {p & 0xff, ab ? (p >> 8) & 0xff : 0, ab ? (unsigned)(p >> 16) & 0xffu : 0u, (unsigned)(p >> 24) & 1u};
}

// The shape of a wave-per-block launch: waves per SIMD, blocks per wavefront, prefetch (fl_widths.hpp).  Each family's default comes
// from fl_dispatch.hpp; with_policy lays the A/B tools' overrides over it (the launcher tidies bpw / prefetch: tidy_wave_blocks).
struct WaveShape {
    int waves;
    unsigned bpw = 1, prefetch = 0;
};
inline WaveShape with_policy(WaveShape sh)
{
    const KernelPolicy p = kernel_policy();
    if (p.waves) sh.waves = p.waves;
    if (p.bpw) { sh.bpw = p.bpw; sh.prefetch = p.prefetch; }
    return sh;
}

// The kernel the policy gives a uniform-width (T, W, op): waves per SIMD for the wave-per-block kernel (0 = the cell-column kernel), and
// whether it takes two blocks per wavefront (fl_dispatch.hpp: wave_choice).  The per-(T,W) cell-column families are only built where
// the table chose them (cell_column_built); Delta's / Transpose's per-type cell-column kernels (no width parameter) always exist.
inline WaveChoice chosen_waves(unsigned type_bits, unsigned w, fl::WaveOp op)
{
    const KernelPolicy p = kernel_policy();
    const WaveChoice table = fl::wave_choice(type_bits, w, op);
    const bool per_type = op == fl::WAVE_UNDELTA || op == fl::WAVE_DELTA || op == fl::WAVE_TRANSPOSE || op == fl::WAVE_UNTRANSPOSE;
    if (p.mode == 1) return (per_type || fl::cell_column_built(type_bits, w, op)) ? WaveChoice{0, false} : table;
    if (p.mode != 2) return table;
    const bool pack = op == fl::WAVE_PACK || op == fl::WAVE_FOR_PACK || op == fl::WAVE_TRANSPOSE_DELTA_PACK;
    WaveChoice c = p.waves ? WaveChoice{p.waves, false} : table.waves ? table : WaveChoice{fl::wave_fallback(type_bits, pack), false};
    if (p.bpw) c.two_blocks = p.bpw == 2;         // the A/B tools force either form: 2 + 256 * waves + 65536 * {1, 2}
    return c;
}

template <typename T>
int run_stream(stream_launch_t fn, const T* in, T* out, const void* aux, size_t aux_stride,
               size_t n_blocks, bool need_in, bool need_out, bool need_aux, void* stream)
{
    if (n_blocks == 0) return FL_OK;
    if ((need_in && !in) || (need_out && !out) || (need_aux && !aux)) return FL_ERR_NULL;
    if (misaligned(in) || misaligned(out)) return FL_ERR_ALIGN;
    // a cell-column instance exists only where the dispatch table sends calls to it (fl_kernels.hpp: unpack_entry / pack_entry);
    // chosen_waves() never selects a missing one, but a table / build mismatch must be an error, not a call through nullptr
    if (!fn) return hip_fail(hipErrorInvalidDeviceFunction);
    StreamArgs a;
    a.in = reinterpret_cast<const u32x4*>(in);
    a.out = reinterpret_cast<u32x4*>(out);
    a.aux = aux;
    a.aux_stride = aux_stride;
    a.n_blocks = n_blocks;
    return hip_status(fn(a, static_cast<hipStream_t>(stream)));
}

// Delta's bodies and the transposes on the wave-per-block pipeline kernel (fl_chain.hpp).  Returns -1 when no such form
// exists for the op: the caller then uses the cell-column kernel.
// Mixed-width form (widths != nullptr; the three ops with a packed side only): per-block widths[] / offsets[] read and checked
// by the kernel, `w` unused.
template <typename T>
int run_chain(int op, int waves, unsigned w, const T* in, const T* bases, T* out, size_t n_blocks, void* stream,
              const uint8_t* widths = nullptr, const uint64_t* offsets = nullptr, size_t packed_bytes = 0, uint32_t* err_flag = nullptr,
              bool two_blocks = false)
{
    fl::chain_launch_t fn = widths ? fl::chain_widths_launcher<T>(op) : fl::chain_launcher<T>(op);
    if (two_blocks && !widths) {                            // the two-blocks-per-wavefront form, where it exists (fl_chain.hpp)
        if (const fl::chain_launch_t fn2 = fl::chain_launcher_two_blocks<T>(op)) fn = fn2;
    }
    if (!fn) return -1;
    if (n_blocks == 0) return FL_OK;
    const bool packed_in = op == fl::OP_UNDELTA_PACK || op == fl::OP_UNDELTA_PACK_UNTRANSPOSE;
    const bool packed_out = op == fl::OP_TRANSPOSE_DELTA_PACK;
    const bool needs_bases = op != fl::OP_TRANSPOSE && op != fl::OP_UNTRANSPOSE;
    if (widths) {
        // a column whose blocks all have width 0 has no packed bytes: its packed pointer may be NULL (run_widths)
        static const T no_bytes[16 / sizeof(T)] __attribute__((aligned(16))) = {0};
        if (packed_bytes == 0 && packed_in && !in) in = no_bytes;
        if (packed_bytes == 0 && packed_out && !out) out = const_cast<T*>(no_bytes);   // never written: every block is skipped or has W = 0
        if (!(packed_in || packed_out) || !offsets) return FL_ERR_NULL;
    }
    if ((!out && !(packed_out && w == 0 && !widths)) || (needs_bases && !bases) || (!(packed_in && w == 0 && !widths) && !in)) return FL_ERR_NULL;
    if (misaligned(in) || misaligned(out) || misaligned(bases)) return FL_ERR_ALIGN;
    fl::ChainArgs a;
    a.in = reinterpret_cast<const char*>(in);
    a.out = reinterpret_cast<char*>(out);
    a.bases = reinterpret_cast<const char*>(bases);
    a.n_blocks = n_blocks;
    a.width = w;
    a.widths = widths;
    a.offsets = offsets;
    a.err_flag = err_flag;
    a.packed_bytes = packed_bytes;
    a.nt_from = fl::nt_read_from(Elem<T>::BITS);
    return hip_status(fn(a, waves, static_cast<hipStream_t>(stream)));
}

// Uniform-width call served by the wave-per-block kernels (fl_dispatch.hpp decides; 0 waves = cell-column kernel).
template <typename T>
int run_wave_uniform(bool pack, int waves, unsigned w, const T* packed, T* unpacked, const T* refs, size_t ref_stride,
                     size_t n_blocks, void* stream)
{
    if (n_blocks == 0 || (pack && w == 0)) return FL_OK;
    if (!unpacked || (w != 0 && !packed)) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(unpacked)) return FL_ERR_ALIGN;
    WidthsArgs a;
    a.packed = reinterpret_cast<const char*>(packed);
    a.unpacked = reinterpret_cast<char*>(unpacked);
    a.widths = nullptr;
    a.offsets = nullptr;
    a.err_flag = nullptr;
    a.refs = refs;
    a.ref_stride = ref_stride;
    a.n_blocks = n_blocks;
    a.uniform_width = w;
    const unsigned bpw = uniform_blocks_per_wave(Elem<T>::BITS, pack, w, refs != nullptr);
    const WaveShape sh = with_policy({waves, bpw, bpw > 1});
    a.bpw = sh.bpw;
    a.packed_bytes = 0;      // not read: uniform-width calls are validated here, on the host side
    a.prefetch = sh.prefetch;
    a.linear_map = 0;
    a.nt_from = fl::nt_read_from(Elem<T>::BITS);
    return hip_status(widths_launcher<T>(pack)(a, sh.waves, static_cast<hipStream_t>(stream)));
}

template <typename T> int dev_pack(unsigned w, const T* in, T* out, size_t n, void* s)
{
    if (w > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (const int waves = chosen_waves(Elem<T>::BITS, w, WAVE_PACK).waves) {
        if (n && !in) return FL_ERR_NULL;
        return run_wave_uniform<T>(true, waves, w, out, const_cast<T*>(in), nullptr, 0, n, s);
    }
    return run_stream<T>(pack_table_impl<T, PACK_PLAIN>().fn[w], in, out, nullptr, 0, n, true, w != 0, false, s);
}
template <typename T> int dev_unpack(unsigned w, const T* in, T* out, size_t n, void* s)
{
    if (w > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (const int waves = chosen_waves(Elem<T>::BITS, w, WAVE_UNPACK).waves)
        return run_wave_uniform<T>(false, waves, w, in, out, nullptr, 0, n, s);
    return run_stream<T>(unpack_table_impl<T, BODY_STORE>().fn[w], in, out, nullptr, 0, n, w != 0, true, false, s);
}
template <typename T>
int dev_for_pack(unsigned w, const T* in, const T* refs, size_t stride, T* out, size_t n, void* s)
{
    if (w > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (const int waves = chosen_waves(Elem<T>::BITS, w, WAVE_FOR_PACK).waves) {
        if (n && (!in || !refs)) return FL_ERR_NULL;
        return run_wave_uniform<T>(true, waves, w, out, const_cast<T*>(in), refs, stride, n, s);
    }
    return run_stream<T>(pack_table_impl<T, PACK_FOR>().fn[w], in, out, refs, stride, n, true, w != 0, true, s);
}
template <typename T>
int dev_unfor_pack(unsigned w, const T* in, const T* refs, size_t stride, T* out, size_t n, void* s)
{
    if (w > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (const int waves = chosen_waves(Elem<T>::BITS, w, WAVE_UNFOR_PACK).waves) {
        if (n && !refs) return FL_ERR_NULL;
        return run_wave_uniform<T>(false, waves, w, in, out, refs, stride, n, s);
    }
    return run_stream<T>(unpack_table_impl<T, BODY_ADD_REF>().fn[w], in, out, refs, stride, n, w != 0, true, true, s);
}
template <typename T>
int dev_undelta_pack(unsigned w, const T* in, const T* bases, T* out, size_t n, void* s)
{
    if (w > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (n && misaligned(bases)) return FL_ERR_ALIGN;
    if (const WaveChoice c = chosen_waves(Elem<T>::BITS, w, WAVE_UNDELTA_PACK); c.waves) {
        const int rc = run_chain<T>(OP_UNDELTA_PACK, c.waves, w, in, bases, out, n, s, nullptr, nullptr, 0, nullptr, c.two_blocks);
        if (rc >= 0) return rc;                  // -1: no pipeline form of this op (cannot happen today): the cell-column kernel
    }
    return run_stream<T>(unpack_table_impl<T, BODY_UNDELTA>().fn[w], in, out, bases, 0, n, w != 0, true, true, s);
}
template <typename T>
int dev_undelta_pack_untranspose(unsigned w, const T* in, const T* bases, T* out, size_t n, void* s)
{
    if (w > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (n && misaligned(bases)) return FL_ERR_ALIGN;
    if (const int waves = chosen_waves(Elem<T>::BITS, w, WAVE_UNDELTA_PACK_UNTRANSPOSE).waves) {
        const int rc = run_chain<T>(OP_UNDELTA_PACK_UNTRANSPOSE, waves, w, in, bases, out, n, s);
        if (rc >= 0) return rc;
    }
    return run_stream<T>(unpack_table_impl<T, BODY_UNDELTA_UNTRANSPOSE>().fn[w], in, out, bases, 0, n, w != 0, true, true, s);
}
template <typename T>
int dev_transpose_delta_pack(unsigned w, const T* in, const T* bases, T* out, size_t n, void* s)
{
    if (w > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (n && misaligned(bases)) return FL_ERR_ALIGN;
    if (const int waves = chosen_waves(Elem<T>::BITS, w, WAVE_TRANSPOSE_DELTA_PACK).waves) {
        const int rc = run_chain<T>(OP_TRANSPOSE_DELTA_PACK, waves, w, in, bases, out, n, s);
        if (rc >= 0) return rc;
    }
    return run_stream<T>(pack_table_impl<T, PACK_TRANSPOSE_DELTA>().fn[w], in, out, bases, 0, n, true, w != 0, true, s);
}
template <typename T>
int dev_unpack_block_sums(unsigned w, const T* in, size_t n, uint64_t* sums, void* s)
{
    if (w > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (n == 0) return FL_OK;
    if (!sums || (w != 0 && !in)) return FL_ERR_NULL;
    if (misaligned(in)) return FL_ERR_ALIGN;
    ReduceArgs a{reinterpret_cast<const u32x4*>(in), sums, nullptr, n};
    return hip_status(sum_table_impl<T>().fn[w](a, static_cast<hipStream_t>(s)));
}
template <typename T>
int dev_unpack_compare(unsigned w, const T* in, int op, T constant, size_t n, uint32_t* mask, void* s)
{
    if (w > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (op < FL_CMP_EQ || op > FL_CMP_GE) return FL_ERR_INDEX;
    if (n == 0) return FL_OK;
    if (!mask || (w != 0 && !in)) return FL_ERR_NULL;
    if (misaligned(in) || misaligned(mask)) return FL_ERR_ALIGN;
    // reduce the six predicates to  x == k  /  x <= k  plus a complement
    const T MAXV = (T) ~(T)0;
    CompareArgs a;
    a.in = reinterpret_cast<const u32x4*>(in);
    a.mask = reinterpret_cast<u32x4*>(mask);
    a.n_blocks = n;
    a.is_eq = 0;
    a.invert = 0;
    a.constant = constant;
    switch (op) {
    case FL_CMP_EQ: a.is_eq = 1; break;
    case FL_CMP_NE: a.is_eq = 1; a.invert = 1; break;
    case FL_CMP_LE: break;
    case FL_CMP_GT: a.invert = 1; break;
    case FL_CMP_LT:                       // x < k  ==  x <= k-1 ;  x < 0 is never true
        if (constant == 0) { a.constant = MAXV; a.invert = 1; } else a.constant = (T)(constant - 1);
        break;
    default:                              // FL_CMP_GE: x >= k == !(x <= k-1) ; x >= 0 is always true
        if (constant == 0) a.constant = MAXV; else { a.constant = (T)(constant - 1); a.invert = 1; }
        break;
    }
    const int waves = with_policy({compare_launch_waves(Elem<T>::BITS, w)}).waves;
    return hip_status((a.is_eq ? compare_table_impl<T, true>() : compare_table_impl<T, false>()).fn[w](a, waves, static_cast<hipStream_t>(s)));
}
template <typename T>
int dev_block_min_max(const T* in, size_t n, T* mins, T* maxs, void* s)
{
    if (n == 0) return FL_OK;
    if (!in || !mins || !maxs) return FL_ERR_NULL;
    if (misaligned(in)) return FL_ERR_ALIGN;
    ReduceArgs a{reinterpret_cast<const u32x4*>(in), mins, maxs, n};
    return hip_status(min_max_launcher<T>()(a, static_cast<hipStream_t>(s)));
}
template <typename T> int dev_delta(bool inverse, const T* in, const T* bases, T* out, size_t n, void* s)
{
    if (n && misaligned(bases)) return FL_ERR_ALIGN;
    if (const int waves = chosen_waves(Elem<T>::BITS, Elem<T>::BITS, inverse ? WAVE_UNDELTA : WAVE_DELTA).waves) {
        const int rc = run_chain<T>(inverse ? OP_UNDELTA : OP_DELTA, waves, Elem<T>::BITS, in, bases, out, n, s);
        if (rc >= 0) return rc;
    }
    return run_stream<T>(delta_launcher<T>(inverse), in, out, bases, 0, n, true, true, true, s);
}
template <typename T> int dev_transpose(bool inverse, const T* in, T* out, size_t n, void* s)
{
    if (const int waves = chosen_waves(Elem<T>::BITS, Elem<T>::BITS, inverse ? WAVE_UNTRANSPOSE : WAVE_TRANSPOSE).waves) {
        const int rc = run_chain<T>(inverse ? OP_UNTRANSPOSE : OP_TRANSPOSE, waves, Elem<T>::BITS, in, static_cast<const T*>(nullptr), out, n, s);
        if (rc >= 0) return rc;
    }
    return run_stream<T>(transpose_launcher<T>(inverse), in, out, nullptr, 0, n, true, true, false, s);
}
template <typename T>
int dev_unpack_single(unsigned w, const T* packed, size_t n_blocks, const uint64_t* idx, size_t n_idx,
                      T* out, uint32_t* err_flag, void* s)
{
    if (w > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (n_idx == 0) return FL_OK;
    if (!idx || !out || (w != 0 && !packed)) return FL_ERR_NULL;
    SingleArgs a{packed, idx, out, err_flag, n_blocks, n_idx, w, nullptr, nullptr, 0};
    return hip_status(unpack_single_launch<T>(a, static_cast<hipStream_t>(s)));
}

template <typename T>
int dev_unpack_single_widths(const uint8_t* widths, const uint64_t* offsets, const T* packed, size_t packed_bytes, size_t n_blocks,
                             const uint64_t* idx, size_t n_idx, T* out, uint32_t* err_flag, void* s)
{
    if (n_idx == 0) return FL_OK;
    static const T no_bytes[16 / sizeof(T)] __attribute__((aligned(16))) = {0};
    if (!packed && packed_bytes == 0) packed = no_bytes;      // a column of width-0 blocks has no packed bytes (every lookup is 0)
    if (!widths || !offsets || !idx || !out || !packed) return FL_ERR_NULL;
    SingleArgs a{packed, idx, out, err_flag, n_blocks, n_idx, 0, widths, offsets, packed_bytes};
    return hip_status(unpack_single_launch<T>(a, static_cast<hipStream_t>(s)));
}

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
    if (w > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
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

// ---------------------------------------------------------------------------
// mixed-width columns: device-resident widths[] / offsets[] (fl_widths.hpp)
// ---------------------------------------------------------------------------
struct fl_mixed_plan {
    unsigned type_bits = 0;
    size_t n_blocks = 0;
    uint64_t packed_bytes = 0;
    uint8_t* d_widths = nullptr;     // widths[n_blocks] in HBM
    uint64_t* d_offsets = nullptr;   // byte offset of every block in the packed column (exclusive prefix sum of 128*W)
};

namespace {

template <typename T>
int run_widths(bool pack, const uint8_t* widths, const uint64_t* offsets, const void* packed, size_t packed_bytes, void* unpacked,
               size_t n_blocks, uint32_t* err_flag, void* stream, const T* refs = nullptr, size_t ref_stride = 0, bool with_refs = false)
{
    if (n_blocks == 0) return FL_OK;
    if (with_refs && !refs) return FL_ERR_NULL;
    // a column whose blocks all have width 0 has no packed bytes at all: its packed pointer may be NULL (any block with a
    // width > 0 then fails the kernel's bounds check against packed_bytes == 0)
    static const char no_bytes[16] __attribute__((aligned(16))) = {0};
    if (!packed && packed_bytes == 0) packed = no_bytes;
    if (!widths || !offsets || !packed || !unpacked) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(unpacked)) return FL_ERR_ALIGN;
    WidthsArgs a;
    a.packed = static_cast<const char*>(packed);
    a.unpacked = static_cast<char*>(unpacked);
    a.widths = widths;
    a.offsets = offsets;
    a.err_flag = err_flag;
    a.refs = with_refs ? refs : nullptr;
    a.ref_stride = ref_stride;
    a.n_blocks = n_blocks;
    a.uniform_width = 0;
    a.packed_bytes = packed_bytes;
    const WaveShape sh = with_policy({mixed_waves(Elem<T>::BITS, pack), mixed_blocks_per_wave(Elem<T>::BITS, pack), mixed_prefetch(Elem<T>::BITS)});
    a.bpw = sh.bpw;
    a.prefetch = sh.prefetch;
    a.linear_map = 0;
    a.nt_from = 0;           // a mixed-width column always streams
    return hip_status(widths_launcher<T>(pack)(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// Delta over a mixed-width column: the pipeline kernel with per-block widths[] / offsets[] on its packed side (fl_chain.hpp)
template <typename T>
int run_chain_widths(int op, const uint8_t* widths, const uint64_t* offsets, const T* in, const T* bases, T* out, size_t packed_bytes,
                     size_t n_blocks, uint32_t* err_flag, void* stream)
{
    if (n_blocks == 0) return FL_OK;
    if (!widths || !offsets) return FL_ERR_NULL;
    // u8 runs the persistent pipelined kernels: 0 = their own grid
    const int waves = with_policy({sizeof(T) == 1 ? 0 : mixed_waves(Elem<T>::BITS, op == OP_TRANSPOSE_DELTA_PACK)}).waves;
    const int rc = run_chain<T>(op, waves, 0, in, bases, out, n_blocks, stream, widths, offsets, packed_bytes, err_flag);
    return rc >= 0 ? rc : hip_fail(hipErrorInvalidDeviceFunction);
}

// The four consumers of a FoR-packed column (fl_for_block.hpp): unfor_compare, unfor_compare_range, unfor_select, unfor_aggregate, each over
// a uniform-width column (mixed = false: `width`, blocks back to back) or a mixed-width one (widths[] / offsets[], checked per block by the
// kernel).  16 aligned zero bytes stand in for a buffer that has none.
template <typename T> const T* no_bytes()
{
    static const T zeros[16 / sizeof(T)] __attribute__((aligned(16))) = {0};
    return zeros;
}
// false: one of the column's pointers is missing (FL_ERR_NULL).  A mixed-width column whose blocks all have width 0 has no packed bytes:
// its packed pointer may be NULL (run_widths) and is replaced here.
template <typename T>
bool block_consumer_column(bool mixed, unsigned width, const uint8_t* widths, const uint64_t* offsets, const T*& packed, size_t packed_bytes, const T* refs)
{
    if (mixed && !packed && packed_bytes == 0) packed = no_bytes<T>();
    return refs && (!mixed || (widths && offsets)) && (packed || (!mixed && width == 0));
}
// the WidthsArgs part of the four argument blocks, launched with the shape of unfor_pack_widths: the same blocks, the same reads
template <typename T>
WaveShape block_consumer_args(WidthsArgs& a, bool mixed, unsigned width, const uint8_t* widths, const uint64_t* offsets, const T* packed,
                              size_t packed_bytes, size_t ref_stride, size_t n_blocks, uint32_t* err_flag)
{
    a.packed = reinterpret_cast<const char*>(packed);
    a.unpacked = nullptr;
    a.widths = mixed ? widths : nullptr;
    a.offsets = mixed ? offsets : nullptr;
    a.err_flag = err_flag;
    a.refs = nullptr;                        // the kernel loads the references with the block's metadata
    a.ref_stride = ref_stride;
    a.n_blocks = n_blocks;
    a.uniform_width = mixed ? 0u : width;
    a.packed_bytes = mixed ? packed_bytes : 0;   // a uniform-width call is validated on the host side
    const WaveShape sh = with_policy({mixed_waves(Elem<T>::BITS, false), mixed_blocks_per_wave(Elem<T>::BITS, false), mixed_prefetch(Elem<T>::BITS)});
    a.bpw = sh.bpw;
    a.prefetch = sh.prefetch;
    a.linear_map = 0;
    a.nt_from = mixed ? 0u : fl::nt_read_from(Elem<T>::BITS);   // a mixed-width column always streams
    return sh;
}

// unfor_compare over a uniform-width column (mixed = false: `width`, blocks back to back) or a mixed-width one (widths[] / offsets[],
// checked per block by the kernel); fl_for_compare.hpp.  The predicate becomes its cyclic interval here, once per call.
template <typename T>
int run_unfor_compare(bool mixed, unsigned width, const uint8_t* widths, const uint64_t* offsets, const T* packed, size_t packed_bytes,
                      const T* refs, size_t ref_stride, int op, T constant, size_t n_blocks, uint32_t* mask, uint32_t* err_flag,
                      void* stream)
{
    if (!mixed && width > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (op < FL_CMP_EQ || op > FL_CMP_GE) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (!block_consumer_column(mixed, width, widths, offsets, packed, packed_bytes, refs) || !mask) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(mask)) return FL_ERR_ALIGN;
    const ForPredicate p = for_compare_predicate(Elem<T>::BITS, op, constant);
    ForCompareArgs a;
    const WaveShape sh = block_consumer_args<T>(a, mixed, width, widths, offsets, packed, packed_bytes, ref_stride, n_blocks, mixed ? err_flag : nullptr);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = refs;
    a.cmp_a = p.a;
    a.cmp_s = p.s;
    a.cmp_none = p.none ? 1u : 0u;
    return hip_status(for_compare_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_compare_range over a uniform-width column (mixed = false) or a mixed-width one: run_unfor_compare with the cyclic interval
// [lo, hi] as the predicate and the mask so far beside it (fl_for_compare_range.hpp).  The same launch shape, the same checks in the
// same order; `mask` may be `mask_in`.
template <typename T>
int run_unfor_compare_range(bool mixed, unsigned width, const uint8_t* widths, const uint64_t* offsets, const T* packed, size_t packed_bytes,
                            const T* refs, size_t ref_stride, T lo, T hi, int combine, const uint32_t* mask_in, size_t n_blocks,
                            uint32_t* mask, uint32_t* err_flag, void* stream)
{
    if (!mixed && width > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (combine < FL_MASK_NEW || combine > FL_MASK_OR) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (combine == FL_MASK_NEW) mask_in = nullptr;                       // ignored: never read, never checked
    else if (!mask_in) return FL_ERR_NULL;
    if (!block_consumer_column(mixed, width, widths, offsets, packed, packed_bytes, refs) || !mask) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(mask) || misaligned(mask_in)) return FL_ERR_ALIGN;
    const ForPredicate p = for_range_predicate(Elem<T>::BITS, lo, hi);
    ForRangeArgs a;
    const WaveShape sh = block_consumer_args<T>(a, mixed, width, widths, offsets, packed, packed_bytes, ref_stride, n_blocks, mixed ? err_flag : nullptr);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = refs;
    a.cmp_a = p.a;
    a.cmp_s = p.s;
    a.cmp_none = 0u;
    a.mask_in = reinterpret_cast<const char*>(mask_in);
    a.combine = (unsigned)combine;
    return hip_status(for_range_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_select over a uniform-width column (mixed = false) or a mixed-width one (widths[] / offsets[], checked per block by the kernel);
// fl_select.hpp.  Launched with the shape of unfor_pack_widths, as unfor_compare is.
template <typename T>
int run_unfor_select(bool mixed, unsigned width, const uint8_t* widths, const uint64_t* offsets, const T* packed, size_t packed_bytes,
                     const T* refs, size_t ref_stride, const uint32_t* mask, const uint64_t* out_offsets, T* out, size_t out_len,
                     size_t n_blocks, uint32_t* err_flag, void* stream)
{
    if (!mixed && width > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (n_blocks == 0) return FL_OK;
    // a selection that keeps nothing has no output: `out` may be NULL with out_len == 0 (a non-empty block then fails the kernel's
    // bounds check; nothing is ever written through this pointer)
    if (!out && out_len == 0) out = const_cast<T*>(no_bytes<T>());
    if (!block_consumer_column(mixed, width, widths, offsets, packed, packed_bytes, refs) || !mask || !out_offsets || !out) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(mask) || misaligned(out)) return FL_ERR_ALIGN;
    SelectArgs a;
    const WaveShape sh = block_consumer_args<T>(a, mixed, width, widths, offsets, packed, packed_bytes, ref_stride, n_blocks, err_flag);   // the uniform form raises FL_DEVERR_BOUNDS too (a run outside `out`)
    a.mask = mask;
    a.out_offsets = out_offsets;
    a.out = reinterpret_cast<char*>(out);
    a.out_len = out_len;
    a.sel_refs = refs;
    return hip_status(select_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_aggregate over a uniform-width column (mixed = false) or a mixed-width one (widths[] / offsets[], checked per block by the kernel:
// a failing block's slot receives the identity); fl_aggregate.hpp.  Launched with the shape of unfor_pack_widths, as unfor_select is.
// `mask` may be NULL: every row is kept and no mask is read.
template <typename T>
int run_unfor_aggregate(bool mixed, unsigned width, const uint8_t* widths, const uint64_t* offsets, const T* packed, size_t packed_bytes,
                        const T* refs, size_t ref_stride, const uint32_t* mask, size_t n_blocks, void* block_aggs, uint32_t* err_flag,
                        void* stream)
{
    if (!mixed && width > (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (n_blocks == 0) return FL_OK;
    if (!block_consumer_column(mixed, width, widths, offsets, packed, packed_bytes, refs) || !block_aggs) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(mask) || misaligned(block_aggs)) return FL_ERR_ALIGN;
    AggregateArgs a;
    const WaveShape sh = block_consumer_args<T>(a, mixed, width, widths, offsets, packed, packed_bytes, ref_stride, n_blocks, mixed ? err_flag : nullptr);
    a.mask = mask;
    a.aggs = static_cast<char*>(block_aggs);
    a.agg_refs = refs;
    return hip_status(aggregate_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

template <typename T> int dev_for_widths(const T* mins, const T* maxs, size_t n, uint8_t* widths, void* s)
{
    if (n == 0) return FL_OK;
    if (!mins || !maxs || !widths) return FL_ERR_NULL;
    return hip_status(launch_for_widths<T>(mins, maxs, n, widths, static_cast<hipStream_t>(s)));
}

// many small arrays, device arrays of pointers (fl_batch.hpp)
template <typename T>
int run_batch(bool pack, const void* const* packed, void* const* unpacked, const uint8_t* widths, const void* refs, bool with_refs,
              const uint32_t* n_blocks, size_t n_arrays, uint32_t max_blocks, uint32_t* err_flag, void* stream)
{
    if (n_arrays == 0 || max_blocks == 0) return FL_OK;
    if (!packed || !unpacked || !widths || !n_blocks || (with_refs && !refs)) return FL_ERR_NULL;
    if (max_blocks > BATCH_MAX_BLOCKS) return FL_ERR_INDEX;       // 2^30 blocks = 2^40 values in ONE array: a bound nobody means
    BatchArgs b;
    b.packed = reinterpret_cast<const char* const*>(packed);
    b.unpacked = reinterpret_cast<char* const*>(unpacked);
    b.widths = widths;
    b.n_blocks = n_blocks;
    b.err_flag = err_flag;
    b.refs = with_refs ? refs : nullptr;
    b.bases = nullptr;
    b.n_arrays = n_arrays;
    b.tiles_per_array = 0;
    b.max_blocks = max_blocks;
    const unsigned bpw = batch_blocks_per_wave(Elem<T>::BITS, pack);
    const WaveShape sh = with_policy({batch_waves(Elem<T>::BITS, pack), bpw, bpw > 1});
    b.bpw = sh.bpw;
    b.prefetch = sh.prefetch;
    return hip_status(batch_launcher<T>(pack)(b, max_blocks, sh.waves, static_cast<hipStream_t>(stream)));
}

// Delta over many small arrays (fl_batch.hpp: k_batch_chain)
template <typename T>
int run_batch_chain(int op, const void* const* packed, const void* const* bases, void* const* unpacked, const uint8_t* widths,
                    const uint32_t* n_blocks, size_t n_arrays, uint32_t max_blocks, uint32_t* err_flag, void* stream)
{
    if (n_arrays == 0 || max_blocks == 0) return FL_OK;
    if (!packed || !bases || !unpacked || !widths || !n_blocks) return FL_ERR_NULL;
    if (max_blocks > BATCH_MAX_BLOCKS) return FL_ERR_INDEX;
    const batch_launch_t fn = batch_chain_launcher<T>(op);
    if (!fn) return hip_fail(hipErrorInvalidDeviceFunction);
    BatchArgs b;
    b.packed = reinterpret_cast<const char* const*>(packed);
    b.unpacked = reinterpret_cast<char* const*>(unpacked);
    b.widths = widths;
    b.n_blocks = n_blocks;
    b.err_flag = err_flag;
    b.refs = nullptr;
    b.bases = reinterpret_cast<const char* const*>(bases);
    b.n_arrays = n_arrays;
    b.tiles_per_array = 0;
    b.max_blocks = max_blocks;
    b.bpw = 1;
    b.prefetch = 0;
    const int waves = with_policy({mixed_waves(Elem<T>::BITS, op == OP_TRANSPOSE_DELTA_PACK)}).waves;
    return hip_status(fn(b, max_blocks, waves, static_cast<hipStream_t>(stream)));
}

template <typename T>
int run_mixed(bool pack, const fl_mixed_plan* p, const void* packed, void* unpacked, void* stream)
{
    if (!p) return FL_ERR_NULL;
    if (p->type_bits != (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (p->n_blocks == 0) return FL_OK;
    if (!unpacked || (p->packed_bytes && !packed)) return FL_ERR_NULL;
    // widths were validated at plan creation; an all-zero-width column has no packed bytes at all (run_widths accepts NULL then)
    return run_widths<T>(pack, p->d_widths, p->d_offsets, p->packed_bytes ? packed : nullptr, p->packed_bytes, unpacked, p->n_blocks, nullptr, stream);
}

}  // namespace

extern "C" {

int fl_widths_to_offsets(unsigned type_bits, const uint8_t* widths, size_t n_blocks, uint64_t* offsets,
                         uint64_t* total_bytes, uint32_t* err_flag, void* stream)
{
    if (type_bits != 8 && type_bits != 16 && type_bits != 32 && type_bits != 64) return FL_ERR_WIDTH;
    if (n_blocks && (!widths || !offsets)) return FL_ERR_NULL;
    FL_DEVICE_TIER(stream, widths, offsets, total_bytes, err_flag);
    ScanArgs a{widths, offsets, total_bytes, err_flag, n_blocks, type_bits};
    return hip_status(launch_widths_to_offsets(a, static_cast<hipStream_t>(stream)));
}

int fl_mask_offsets(const uint32_t* mask, size_t n_blocks, uint64_t* out_offsets, uint64_t* total, void* stream)
{
    if (n_blocks && (!mask || !out_offsets)) return FL_ERR_NULL;
    if (n_blocks && misaligned(mask)) return FL_ERR_ALIGN;
    FL_DEVICE_TIER(stream, mask, out_offsets, total);
    return hip_status(launch_mask_offsets(mask, n_blocks, out_offsets, total, static_cast<hipStream_t>(stream)));
}

int fl_aggregate_reduce(const void* block_aggs, size_t n_blocks, void* result, void* stream)
{
    if (!result || (n_blocks && !block_aggs)) return FL_ERR_NULL;
    if ((n_blocks && misaligned(block_aggs)) || misaligned(result)) return FL_ERR_ALIGN;
    FL_DEVICE_TIER(stream, block_aggs, result);
    return hip_status(launch_aggregate_reduce(static_cast<const BlockAggregate*>(block_aggs), n_blocks, static_cast<BlockAggregate*>(result),
                                              static_cast<hipStream_t>(stream)));
}

int fl_mixed_plan_create(unsigned type_bits, const uint8_t* widths, size_t n_blocks, fl_mixed_plan** plan)
{
    if (!plan || (n_blocks && !widths)) return FL_ERR_NULL;
    *plan = nullptr;
    if (type_bits != 8 && type_bits != 16 && type_bits != 32 && type_bits != 64) return FL_ERR_WIDTH;
    for (size_t b = 0; b < n_blocks; ++b)
        if (widths[b] > type_bits) return FL_ERR_WIDTH;   // bitpacking.rs:93 unreachable!()
    fl_mixed_plan* p = new (std::nothrow) fl_mixed_plan;
    if (!p) { g_last_hip_error = (int)hipErrorOutOfMemory; return FL_ERR_HIP; }
    p->type_bits = type_bits;
    p->n_blocks = n_blocks;
    if (n_blocks) {
        uint64_t* d_total = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_widths), n_blocks);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p->d_offsets), (n_blocks + 1) * sizeof(uint64_t));
        if (e == hipSuccess) {
            d_total = p->d_offsets + n_blocks;             // the total rides behind the offsets: one allocation less
            e = hipMemcpy(p->d_widths, widths, n_blocks, hipMemcpyHostToDevice);
        }
        if (e == hipSuccess) {
            ScanArgs a{p->d_widths, p->d_offsets, d_total, nullptr, n_blocks, type_bits};
            e = launch_widths_to_offsets(a, nullptr);
        }
        if (e == hipSuccess) e = hipMemcpy(&p->packed_bytes, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            fl_mixed_plan_destroy(p);
            return hip_fail(e);
        }
    }
    *plan = p;
    return FL_OK;
}

int fl_fill_random(void* dst, size_t n_bytes, uint64_t seed, void* stream)
{
    if (n_bytes == 0) return FL_OK;
    if (!dst) return FL_ERR_NULL;
    if ((reinterpret_cast<uintptr_t>(dst) & 7u) || (n_bytes & 7u)) return FL_ERR_ALIGN;
    FL_DEVICE_TIER(stream, dst);
    return hip_status(launch_fill_random(static_cast<uint64_t*>(dst), n_bytes / 8, seed, static_cast<hipStream_t>(stream)));
}

// ---- the bare stream (fl_stream.hpp) and the launch shape the library gives an op -----------------------------------------------
int fl_internal_bare_stream(const void* in, size_t in_unit, const void* aux, size_t aux_unit, void* out, size_t out_unit, size_t n_units,
                            int nt_loads, int waves, int window_log2_units, void* stream)
{
    if (n_units == 0) return FL_OK;
    if ((in_unit && !in) || (aux_unit && !aux) || !out) return FL_ERR_NULL;
    if (misaligned(in) || misaligned(aux) || misaligned(out)) return FL_ERR_ALIGN;
    if (in_unit > BARE_MAX_UNIT || out_unit > BARE_MAX_UNIT || aux_unit > 1024 || ((in_unit | out_unit | aux_unit) & 15u)) return FL_ERR_INDEX;
    FL_DEVICE_TIER(stream, in, aux, out);
    BareArgs a{static_cast<const char*>(in), static_cast<const char*>(aux), static_cast<char*>(out), n_units, 0,
               (unsigned)in_unit, (unsigned)aux_unit, (unsigned)out_unit, 63u};
    return hip_status(launch_bare_stream(a, nt_loads != 0, waves, window_log2_units, static_cast<hipStream_t>(stream)));
}

// op: 0 unpack / unfor_pack, 1 pack / for_pack, 2 undelta_pack, 3 unpack over a mixed-width column (width = the column's mean width
// times 2, so that 16.5 can be said).  The shape a bare stream must have to shadow that call: bytes per block on either side, the
// cache policy of the loads, waves per SIMD and tile-map window the library's own kernel for that (T, W) runs with.
int fl_internal_bare_stream_shape(int op, unsigned type_bits, unsigned width, size_t* in_unit, size_t* aux_unit, size_t* out_unit,
                                  int* nt_loads, int* waves, int* window_log2_units, unsigned* blocks_per_unit)
{
    if (type_bits != 8 && type_bits != 16 && type_bits != 32 && type_bits != 64) return FL_ERR_INDEX;
    if (op < 0 || op > 3) return FL_ERR_INDEX;
    if (width > (op == 3 ? 2 * type_bits : type_bits)) return FL_ERR_WIDTH;
    if (!in_unit || !aux_unit || !out_unit || !nt_loads || !waves || !window_log2_units || !blocks_per_unit) return FL_ERR_NULL;
    // a wavefront's unit is at least 4 KiB of unpacked values: 4 consecutive u8 blocks, 2 u16 blocks -- the library's own kernels never
    // give a wavefront a single 1- or 2-KiB block either (8 blocks per wavefront in the cell-column kernels, 2-4 in flight in the others),
    // and a stream that did would measure the starving wavefront, not the memory
    const unsigned k = type_bits == 8 ? 4u : type_bits == 16 ? 2u : 1u;
    const size_t packed = (op == 3 ? 64u * width : 128u * width) * k, unpacked = 128u * type_bits * k;
    *blocks_per_unit = k;
    *in_unit = op == 1 ? unpacked : packed;
    *out_unit = op == 1 ? packed : unpacked;
    *aux_unit = op == 2 ? 128u * k : 0;
    const WaveOp wop = op == 1 ? WAVE_PACK : op == 2 ? WAVE_UNDELTA_PACK : WAVE_UNPACK;
    // two blocks per wavefront: same bytes per launch, the occupancy is what the table says
    int w = op == 3 ? mixed_waves(type_bits, false) : chosen_waves(type_bits, width, wop).waves;
    if (w == 0) w = 8;       // a cell-column kernel gives a wavefront 8 blocks at 2-3 waves per SIMD: the one-unit-per-wavefront stream needs every slot to keep as many bytes in flight
    *waves = w < 3 ? 3 : w;
    *nt_loads = op == 1 || op == 3 || width >= fl::nt_read_from(type_bits);       // fl_widths.hpp: RD_AUTO; pack reads non-temporally
    *window_log2_units = window_log2_blocks(op == 1 ? WIN_PACK : op == 2 ? WIN_UNDELTA_PACK : WIN_UNPACK, type_bits);
    return FL_OK;
}

int fl_internal_selftune_check(int op, unsigned type_bits, unsigned width, const void* in, const void* aux, void* out, size_t n_blocks, void* stream,
                               float* table_ms, float* best_other_ms, int* best_other_policy)
{
    if (!table_ms || !best_other_ms || !best_other_policy) return FL_ERR_NULL;
    if (op < 0 || op > 2 || (type_bits != 8 && type_bits != 16 && type_bits != 32 && type_bits != 64)) return FL_ERR_INDEX;
    if (width > type_bits) return FL_ERR_WIDTH;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto call = [&]() -> int {
        switch (type_bits * 4 + (unsigned)op) {
        case 8 * 4 + 0: return fl_u8_unpack(width, (const uint8_t*)in, (uint8_t*)out, n_blocks, stream);
        case 8 * 4 + 1: return fl_u8_pack(width, (const uint8_t*)in, (uint8_t*)out, n_blocks, stream);
        case 8 * 4 + 2: return fl_u8_undelta_pack(width, (const uint8_t*)in, (const uint8_t*)aux, (uint8_t*)out, n_blocks, stream);
        case 16 * 4 + 0: return fl_u16_unpack(width, (const uint16_t*)in, (uint16_t*)out, n_blocks, stream);
        case 16 * 4 + 1: return fl_u16_pack(width, (const uint16_t*)in, (uint16_t*)out, n_blocks, stream);
        case 16 * 4 + 2: return fl_u16_undelta_pack(width, (const uint16_t*)in, (const uint16_t*)aux, (uint16_t*)out, n_blocks, stream);
        case 32 * 4 + 0: return fl_u32_unpack(width, (const uint32_t*)in, (uint32_t*)out, n_blocks, stream);
        case 32 * 4 + 1: return fl_u32_pack(width, (const uint32_t*)in, (uint32_t*)out, n_blocks, stream);
        case 32 * 4 + 2: return fl_u32_undelta_pack(width, (const uint32_t*)in, (const uint32_t*)aux, (uint32_t*)out, n_blocks, stream);
        case 64 * 4 + 0: return fl_u64_unpack(width, (const uint64_t*)in, (uint64_t*)out, n_blocks, stream);
        case 64 * 4 + 1: return fl_u64_pack(width, (const uint64_t*)in, (uint64_t*)out, n_blocks, stream);
        default: return fl_u64_undelta_pack(width, (const uint64_t*)in, (const uint64_t*)aux, (uint64_t*)out, n_blocks, stream);
        }
    };
    const int saved = fl_internal_get_kernel_policy();
    int rc = FL_OK;
    auto timed = [&](int policy, float& ms) {                // median of 3 after one untimed call
        fl_internal_set_kernel_policy(policy);
        rc = median_ms(s, 1, 3, call, &ms);
    };
    *table_ms = *best_other_ms = 0.f;
    timed(0, *table_ms);
    *best_other_policy = 0;
    const fl::WaveOp wop = op == 1 ? fl::WAVE_PACK : op == 2 ? fl::WAVE_UNDELTA_PACK : fl::WAVE_UNPACK;
    const fl::WaveChoice tab = fl::wave_choice(type_bits, width, wop);
    for (int policy : {1, 2 + 256 * 3, 2 + 256 * 4, 2 + 256 * 5, 2 + 256 * 6, 2 + 256 * 8}) {
        if (rc != FL_OK) break;
        if (policy == 1 && (tab.waves == 0 || !fl::cell_column_built(type_bits, width, wop))) continue;   // the table's own choice, or not built
        if (policy != 1 && (policy >> 8) == tab.waves && !tab.two_blocks) continue;   // the table's own choice
        float ms = 0.f;
        timed(policy, ms);
        if (rc == FL_OK && ms > 0.f && (*best_other_ms == 0.f || ms < *best_other_ms)) { *best_other_ms = ms; *best_other_policy = policy; }
    }
    fl_internal_set_kernel_policy(saved);
    return rc;
}

void fl_mixed_plan_destroy(fl_mixed_plan* p)
{
    if (!p) return;
    if (p->d_widths) (void)hipFree(p->d_widths);
    if (p->d_offsets) (void)hipFree(p->d_offsets);
    delete p;
}
size_t fl_mixed_plan_n_blocks(const fl_mixed_plan* p) { return p ? p->n_blocks : 0; }
uint64_t fl_mixed_plan_packed_bytes(const fl_mixed_plan* p) { return p ? p->packed_bytes : 0; }
const uint64_t* fl_mixed_plan_offsets(const fl_mixed_plan* p) { return p ? p->d_offsets : nullptr; }
const uint8_t* fl_mixed_plan_widths(const fl_mixed_plan* p) { return p ? p->d_widths : nullptr; }

void fl_host_release(void) { g_host.release(); }
void fl_internal_set_kernel_policy(int policy)
{
    const int mode = policy & 0xff, waves = (policy >> 8) & 0xff, bpw = (policy >> 16) & 0xff, prefetch = (policy >> 24) & 1,
              window = (policy >> 25) & 31;
    const bool ok = policy >= 0 && policy < (1 << 30) && mode <= 2 && (waves == 0 || (waves >= 3 && waves <= 8)) && bpw <= 16
                    && (mode == 2 || (waves == 0 && bpw == 0)) && (prefetch == 0 || bpw >= 2) && (window == 0 || window >= 8);
    g_kernel_policy.store(ok ? policy : 0, std::memory_order_relaxed);
    fl::window_override().store(ok ? window : 0, std::memory_order_relaxed);
}
int fl_internal_get_kernel_policy(void) { return g_kernel_policy.load(std::memory_order_relaxed); }
uint64_t fl_internal_zero_copy_fallbacks(void) { return g_zero_copy_fallbacks.load(std::memory_order_relaxed); }

#ifdef FL_ALL_CELL_COLUMN
const char* fl_version(void) { return "fastlanes_amd 0.6.0 (gfx950; wire format of spiraldb/fastlanes 0.1.8; FULL build: every cell-column instance, for A/B sweeps)"; }
#else
const char* fl_version(void) { return "fastlanes_amd 0.6.0 (gfx950; wire format of spiraldb/fastlanes 0.1.8)"; }
#endif

const char* fl_status_string(int status)
{
    switch (status) {
    case FL_OK: return "ok";
    case FL_ERR_WIDTH: return "width > T";
    case FL_ERR_INDEX: return "index out of range";
    case FL_ERR_NULL: return "null pointer";
    case FL_ERR_ALIGN: return "device pointer (or offset / size) not aligned as required";
    case FL_ERR_HIP: return "HIP runtime error";
    case FL_ERR_BOUNDS: return "block outside the packed column";
    case FL_ERR_DEVICE: return "pointer or stream does not belong to the current device (FL_CHECK_DEVICE)";
    default: return "unknown status";
    }
}

int fl_last_hip_error(void) { return g_last_hip_error; }

size_t fl_packed_len(unsigned type_bits, unsigned width)
{
    if (type_bits != 8 && type_bits != 16 && type_bits != 32 && type_bits != 64) return 0;
    if (width > type_bits) return 0;
    return (size_t)1024 * width / type_bits;
}

#define FL_DEFINE_TYPE(T, S)                                                                              \
    int fl_##S##_pack(unsigned w, const T* in, T* out, size_t n, void* s) { FL_DEVICE_TIER(s, in, out); return dev_pack<T>(w, in, out, n, s); } \
    int fl_##S##_unpack(unsigned w, const T* in, T* out, size_t n, void* s) { FL_DEVICE_TIER(s, in, out); return dev_unpack<T>(w, in, out, n, s); } \
    int fl_##S##_unpack_single(unsigned w, const T* pk, size_t n, const uint64_t* idx, size_t ni, T* out,  \
                               uint32_t* ef, void* s)                                                     \
    { FL_DEVICE_TIER(s, pk, idx, out, ef); return dev_unpack_single<T>(w, pk, n, idx, ni, out, ef, s); }                                       \
    int fl_##S##_for_pack(unsigned w, const T* in, const T* r, size_t rs, T* out, size_t n, void* s)      \
    { FL_DEVICE_TIER(s, in, r, out); return dev_for_pack<T>(w, in, r, rs, out, n, s); }                                                  \
    int fl_##S##_unfor_pack(unsigned w, const T* in, const T* r, size_t rs, T* out, size_t n, void* s)    \
    { FL_DEVICE_TIER(s, in, r, out); return dev_unfor_pack<T>(w, in, r, rs, out, n, s); }                                                \
    int fl_##S##_delta(const T* in, const T* b, T* out, size_t n, void* s) { FL_DEVICE_TIER(s, in, b, out); return dev_delta<T>(false, in, b, out, n, s); } \
    int fl_##S##_undelta(const T* in, const T* b, T* out, size_t n, void* s) { FL_DEVICE_TIER(s, in, b, out); return dev_delta<T>(true, in, b, out, n, s); } \
    int fl_##S##_undelta_pack(unsigned w, const T* in, const T* b, T* out, size_t n, void* s)             \
    { FL_DEVICE_TIER(s, in, b, out); return dev_undelta_pack<T>(w, in, b, out, n, s); }                                                  \
    int fl_##S##_undelta_pack_untranspose(unsigned w, const T* in, const T* b, T* out, size_t n, void* s) \
    { FL_DEVICE_TIER(s, in, b, out); return dev_undelta_pack_untranspose<T>(w, in, b, out, n, s); }                                      \
    int fl_##S##_transpose_delta_pack(unsigned w, const T* in, const T* b, T* out, size_t n, void* s)     \
    { FL_DEVICE_TIER(s, in, b, out); return dev_transpose_delta_pack<T>(w, in, b, out, n, s); }                                          \
    int fl_##S##_unpack_block_sums(unsigned w, const T* in, size_t n, uint64_t* sums, void* s)           \
    { FL_DEVICE_TIER(s, in, sums); return dev_unpack_block_sums<T>(w, in, n, sums, s); }                                               \
    int fl_##S##_unpack_compare(unsigned w, const T* in, int op, T k, size_t n, uint32_t* mask, void* s)  \
    { FL_DEVICE_TIER(s, in, mask); return dev_unpack_compare<T>(w, in, op, k, n, mask, s); }                                           \
    int fl_##S##_unfor_compare(unsigned w, const T* in, const T* r, size_t rs, int op, T k, size_t n, uint32_t* mask, void* s) \
    { FL_DEVICE_TIER(s, in, r, mask); return run_unfor_compare<T>(false, w, nullptr, nullptr, in, 0, r, rs, op, k, n, mask, nullptr, s); } \
    int fl_##S##_unfor_compare_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, int op, T k, \
                                      size_t n, uint32_t* mask, uint32_t* ef, void* s)                   \
    { FL_DEVICE_TIER(s, w, o, pk, r, mask, ef); return run_unfor_compare<T>(true, 0, w, o, pk, pb, r, rs, op, k, n, mask, ef, s); }     \
    int fl_##S##_block_min_max(const T* in, size_t n, T* mins, T* maxs, void* s)                          \
    { FL_DEVICE_TIER(s, in, mins, maxs); return dev_block_min_max<T>(in, n, mins, maxs, s); }                                                \
    int fl_##S##_transpose(const T* in, T* out, size_t n, void* s) { FL_DEVICE_TIER(s, in, out); return dev_transpose<T>(false, in, out, n, s); } \
    int fl_##S##_untranspose(const T* in, T* out, size_t n, void* s) { FL_DEVICE_TIER(s, in, out); return dev_transpose<T>(true, in, out, n, s); } \
    int fl_##S##_unpack_mixed(const fl_mixed_plan* p, const T* pk, T* out, void* s) { FL_DEVICE_TIER(s, pk, out); return run_mixed<T>(false, p, pk, out, s); } \
    int fl_##S##_pack_mixed(const fl_mixed_plan* p, const T* in, T* pk, void* s) { FL_DEVICE_TIER(s, in, pk); return run_mixed<T>(true, p, pk, const_cast<T*>(in), s); } \
    int fl_##S##_unpack_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, T* out, size_t n, uint32_t* ef, void* s) \
    { FL_DEVICE_TIER(s, w, o, pk, out, ef); return run_widths<T>(false, w, o, pk, pb, out, n, ef, s); }                                         \
    int fl_##S##_pack_widths(const uint8_t* w, const uint64_t* o, const T* in, T* pk, size_t pb, size_t n, uint32_t* ef, void* s) \
    { FL_DEVICE_TIER(s, w, o, in, pk, ef); return run_widths<T>(true, w, o, pk, pb, const_cast<T*>(in), n, ef, s); }                           \
    int fl_##S##_unfor_pack_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, T* out, \
                                   size_t n, uint32_t* ef, void* s)                                        \
    { FL_DEVICE_TIER(s, w, o, pk, r, out, ef); return run_widths<T>(false, w, o, pk, pb, out, n, ef, s, r, rs, true); }                        \
    int fl_##S##_for_pack_widths(const uint8_t* w, const uint64_t* o, const T* in, const T* r, size_t rs, T* pk, size_t pb, \
                                 size_t n, uint32_t* ef, void* s)                                          \
    { FL_DEVICE_TIER(s, w, o, in, r, pk, ef); return run_widths<T>(true, w, o, pk, pb, const_cast<T*>(in), n, ef, s, r, rs, true); }          \
    int fl_##S##_for_widths(const T* mins, const T* maxs, size_t n, uint8_t* w, void* s)                   \
    { FL_DEVICE_TIER(s, mins, maxs, w); return dev_for_widths<T>(mins, maxs, n, w, s); }                                                      \
    int fl_##S##_undelta_pack_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* b, T* out, size_t n, \
                                     uint32_t* ef, void* s)                                                \
    { FL_DEVICE_TIER(s, w, o, pk, b, out, ef); return run_chain_widths<T>(OP_UNDELTA_PACK, w, o, pk, b, out, pb, n, ef, s); }                  \
    int fl_##S##_undelta_pack_untranspose_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* b, T* out, \
                                                 size_t n, uint32_t* ef, void* s)                          \
    { FL_DEVICE_TIER(s, w, o, pk, b, out, ef); return run_chain_widths<T>(OP_UNDELTA_PACK_UNTRANSPOSE, w, o, pk, b, out, pb, n, ef, s); }      \
    int fl_##S##_transpose_delta_pack_widths(const uint8_t* w, const uint64_t* o, const T* in, const T* b, T* pk, size_t pb, \
                                             size_t n, uint32_t* ef, void* s)                              \
    { FL_DEVICE_TIER(s, w, o, in, b, pk, ef); return run_chain_widths<T>(OP_TRANSPOSE_DELTA_PACK, w, o, in, b, pk, pb, n, ef, s); }            \
    int fl_##S##_unpack_batch(const T* const* pk, T* const* out, const uint8_t* w, const uint32_t* nb, size_t na, uint32_t mb, \
                              uint32_t* ef, void* s)                                                      \
    { FL_DEVICE_TIER(s, pk, out, w, nb, ef); return run_batch<T>(false, reinterpret_cast<const void* const*>(pk), reinterpret_cast<void* const*>(out), w, nullptr, false, nb, na, mb, ef, s); } \
    int fl_##S##_unfor_pack_batch(const T* const* pk, T* const* out, const uint8_t* w, const T* refs, const uint32_t* nb, size_t na, \
                                  uint32_t mb, uint32_t* ef, void* s)                                     \
    { FL_DEVICE_TIER(s, pk, out, w, refs, nb, ef); return run_batch<T>(false, reinterpret_cast<const void* const*>(pk), reinterpret_cast<void* const*>(out), w, refs, true, nb, na, mb, ef, s); } \
    int fl_##S##_for_pack_batch(const T* const* in, T* const* pk, const uint8_t* w, const T* refs, const uint32_t* nb, size_t na, \
                                uint32_t mb, uint32_t* ef, void* s)                                       \
    { FL_DEVICE_TIER(s, pk, in, w, refs, nb, ef); return run_batch<T>(true, reinterpret_cast<const void* const*>(pk), (void* const*)in, w, refs, true, nb, na, mb, ef, s); } \
    int fl_##S##_pack_batch(const T* const* in, T* const* pk, const uint8_t* w, const uint32_t* nb, size_t na, uint32_t mb, \
                            uint32_t* ef, void* s)                                                        \
    { FL_DEVICE_TIER(s, pk, in, w, nb, ef); return run_batch<T>(true, reinterpret_cast<const void* const*>(pk), (void* const*)in, w, nullptr, false, nb, na, mb, ef, s); } \
    int fl_##S##_undelta_pack_batch(const T* const* pk, const T* const* bs, T* const* out, const uint8_t* w, const uint32_t* nb, \
                                    size_t na, uint32_t mb, int untranspose, uint32_t* ef, void* s)        \
    { FL_DEVICE_TIER(s, pk, bs, out, w, nb, ef); return run_batch_chain<T>(untranspose ? OP_UNDELTA_PACK_UNTRANSPOSE : OP_UNDELTA_PACK, reinterpret_cast<const void* const*>(pk), reinterpret_cast<const void* const*>(bs), reinterpret_cast<void* const*>(out), w, nb, na, mb, ef, s); } \
    int fl_##S##_transpose_delta_pack_batch(const T* const* in, const T* const* bs, T* const* pk, const uint8_t* w, const uint32_t* nb, \
                                            size_t na, uint32_t mb, uint32_t* ef, void* s)                 \
    { FL_DEVICE_TIER(s, in, bs, pk, w, nb, ef); return run_batch_chain<T>(OP_TRANSPOSE_DELTA_PACK, reinterpret_cast<const void* const*>(pk), reinterpret_cast<const void* const*>(bs), (void* const*)in, w, nb, na, mb, ef, s); } \
    int fl_##S##_unpack_single_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, size_t n, const uint64_t* idx, \
                                      size_t ni, T* out, uint32_t* ef, void* s)                           \
    { FL_DEVICE_TIER(s, w, o, pk, idx, out, ef); return dev_unpack_single_widths<T>(w, o, pk, pb, n, idx, ni, out, ef, s); }                         \
    int fl_##S##_pack_host(unsigned w, const T* in, T* out, size_t n)                                     \
    {                                                                                                     \
        if (w > sizeof(T) * 8) return FL_ERR_WIDTH;                                                       \
        return host_run<T>(in, n * 1024, nullptr, 0, out, n * plen<T>(w),                                 \
                           [&](const T* di, const T*, T* d_o, void* st) { return dev_pack<T>(w, di, d_o, n, st); }); \
    }                                                                                                     \
    int fl_##S##_unpack_host(unsigned w, const T* in, T* out, size_t n)                                   \
    {                                                                                                     \
        if (w > sizeof(T) * 8) return FL_ERR_WIDTH;                                                       \
        return host_run<T>(in, n * plen<T>(w), nullptr, 0, out, n * 1024,                                 \
                           [&](const T* di, const T*, T* d_o, void* st) { return dev_unpack<T>(w, di, d_o, n, st); }); \
    }                                                                                                     \
    int fl_##S##_unpack_single_host(unsigned w, const T* pk, size_t n, uint64_t index, T* value)          \
    { return host_unpack_single<T>(w, pk, n, index, value); }                                             \
    int fl_##S##_for_pack_host(unsigned w, const T* in, T reference, T* out, size_t n)                    \
    {                                                                                                     \
        if (w > sizeof(T) * 8) return FL_ERR_WIDTH;                                                       \
        return host_run<T>(in, n * 1024, &reference, 1, out, n * plen<T>(w),                              \
                           [&](const T* di, const T* da, T* d_o, void* st) { return dev_for_pack<T>(w, di, da, 0, d_o, n, st); }); \
    }                                                                                                     \
    int fl_##S##_unfor_pack_host(unsigned w, const T* in, T reference, T* out, size_t n)                  \
    {                                                                                                     \
        if (w > sizeof(T) * 8) return FL_ERR_WIDTH;                                                       \
        return host_run<T>(in, n * plen<T>(w), &reference, 1, out, n * 1024,                              \
                           [&](const T* di, const T* da, T* d_o, void* st) { return dev_unfor_pack<T>(w, di, da, 0, d_o, n, st); }); \
    }                                                                                                     \
    int fl_##S##_delta_host(const T* in, const T* b, T* out, size_t n)                                    \
    {                                                                                                     \
        return host_run<T>(in, n * 1024, b, n * (1024 / (sizeof(T) * 8)), out, n * 1024,                  \
                           [&](const T* di, const T* da, T* d_o, void* st) { return dev_delta<T>(false, di, da, d_o, n, st); }); \
    }                                                                                                     \
    int fl_##S##_undelta_host(const T* in, const T* b, T* out, size_t n)                                  \
    {                                                                                                     \
        return host_run<T>(in, n * 1024, b, n * (1024 / (sizeof(T) * 8)), out, n * 1024,                  \
                           [&](const T* di, const T* da, T* d_o, void* st) { return dev_delta<T>(true, di, da, d_o, n, st); }); \
    }                                                                                                     \
    int fl_##S##_undelta_pack_host(unsigned w, const T* in, const T* b, T* out, size_t n)                 \
    {                                                                                                     \
        if (w > sizeof(T) * 8) return FL_ERR_WIDTH;                                                       \
        return host_run<T>(in, n * plen<T>(w), b, n * (1024 / (sizeof(T) * 8)), out, n * 1024,            \
                           [&](const T* di, const T* da, T* d_o, void* st) { return dev_undelta_pack<T>(w, di, da, d_o, n, st); }); \
    }                                                                                                     \
    int fl_##S##_transpose_host(const T* in, T* out, size_t n)                                            \
    {                                                                                                     \
        return host_run<T>(in, n * 1024, nullptr, 0, out, n * 1024,                                       \
                           [&](const T* di, const T*, T* d_o, void* st) { return dev_transpose<T>(false, di, d_o, n, st); }); \
    }                                                                                                     \
    int fl_##S##_untranspose_host(const T* in, T* out, size_t n)                                          \
    {                                                                                                     \
        return host_run<T>(in, n * 1024, nullptr, 0, out, n * 1024,                                       \
                           [&](const T* di, const T*, T* d_o, void* st) { return dev_transpose<T>(true, di, d_o, n, st); }); \
    }

#define FL_DEFINE_SELECT(T, S)                                                                            \
    int fl_##S##_unfor_select(unsigned w, const T* in, const T* r, size_t rs, const uint32_t* mask, const uint64_t* oo, T* out, size_t ol, \
                              size_t n, uint32_t* ef, void* s)                                            \
    { FL_DEVICE_TIER(s, in, r, mask, oo, out, ef); return run_unfor_select<T>(false, w, nullptr, nullptr, in, 0, r, rs, mask, oo, out, ol, n, ef, s); } \
    int fl_##S##_unfor_select_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, const uint32_t* mask, \
                                     const uint64_t* oo, T* out, size_t ol, size_t n, uint32_t* ef, void* s) \
    { FL_DEVICE_TIER(s, w, o, pk, r, mask, oo, out, ef); return run_unfor_select<T>(true, 0, w, o, pk, pb, r, rs, mask, oo, out, ol, n, ef, s); }

FL_DEFINE_SELECT(uint8_t, u8)
FL_DEFINE_SELECT(uint16_t, u16)
FL_DEFINE_SELECT(uint32_t, u32)
FL_DEFINE_SELECT(uint64_t, u64)

#define FL_DEFINE_AGGREGATE(T, S)                                                                         \
    int fl_##S##_unfor_aggregate(unsigned w, const T* in, const T* r, size_t rs, const uint32_t* mask, size_t n, void* aggs, uint32_t* ef, \
                                 void* s)                                                                 \
    { FL_DEVICE_TIER(s, in, r, mask, aggs, ef); return run_unfor_aggregate<T>(false, w, nullptr, nullptr, in, 0, r, rs, mask, n, aggs, ef, s); } \
    int fl_##S##_unfor_aggregate_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, const uint32_t* mask, \
                                        size_t n, void* aggs, uint32_t* ef, void* s)                      \
    { FL_DEVICE_TIER(s, w, o, pk, r, mask, aggs, ef); return run_unfor_aggregate<T>(true, 0, w, o, pk, pb, r, rs, mask, n, aggs, ef, s); }

FL_DEFINE_AGGREGATE(uint8_t, u8)
FL_DEFINE_AGGREGATE(uint16_t, u16)
FL_DEFINE_AGGREGATE(uint32_t, u32)
FL_DEFINE_AGGREGATE(uint64_t, u64)

#define FL_DEFINE_FOR_COMPARE_RANGE(T, S)                                                                 \
    int fl_##S##_unfor_compare_range(unsigned w, const T* in, const T* r, size_t rs, T lo, T hi, int cb, const uint32_t* mi, size_t n, \
                                     uint32_t* mask, void* s)                                             \
    { FL_DEVICE_TIER(s, in, r, mi, mask); return run_unfor_compare_range<T>(false, w, nullptr, nullptr, in, 0, r, rs, lo, hi, cb, mi, n, mask, nullptr, s); } \
    int fl_##S##_unfor_compare_range_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, T lo, T hi, \
                                            int cb, const uint32_t* mi, size_t n, uint32_t* mask, uint32_t* ef, void* s) \
    { FL_DEVICE_TIER(s, w, o, pk, r, mi, mask, ef); return run_unfor_compare_range<T>(true, 0, w, o, pk, pb, r, rs, lo, hi, cb, mi, n, mask, ef, s); }

FL_DEFINE_FOR_COMPARE_RANGE(uint8_t, u8)
FL_DEFINE_FOR_COMPARE_RANGE(uint16_t, u16)
FL_DEFINE_FOR_COMPARE_RANGE(uint32_t, u32)
FL_DEFINE_FOR_COMPARE_RANGE(uint64_t, u64)

FL_DEFINE_TYPE(uint8_t, u8)
FL_DEFINE_TYPE(uint16_t, u16)
FL_DEFINE_TYPE(uint32_t, u32)
FL_DEFINE_TYPE(uint64_t, u64)

}  // extern "C"
