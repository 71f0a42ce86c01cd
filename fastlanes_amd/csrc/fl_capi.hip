// fl_capi.hip -- the extern "C" boundary declared in include/fastlanes_amd.h.
// Validates arguments, maps the runtime width to the per-(T,W) kernel instance
// (the reference's `match width`, bitpacking.rs:82-95) and launches it.  No CPU
// compute path exists in this library: every entry point ends in a HIP launch.
// In this order: the kernel policy; the builders of the launch-argument blocks and the device tier's validators (run_* / dev_*);
// the consumers of a packed column (fl_consumer_tier.hpp, included where what it builds on is defined); fl_mixed_plan; extern "C" --
// the public entry points, then the fl_internal_* ones of the A/B tools.  Three headers are part of this translation unit alone: the
// host tier (HostCtx, host_run: fl_host_tier.hpp), the scans (fl_scan.hpp) and the consumer tier (fl_consumer_tier.hpp: the host side
// of every consumer of a packed column and its entry points).  fl_column_pair_alloc / _free and the memory-class probe live in
// fl_pair.hip.
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
#include "fl_host_tier.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>
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
    int bpw;              // 0 = the launch's own blocks per wavefront and prefetch
    int prefetch;
    int window;           // 0 = the window table's
};
// THE bit layout.  Only what fl_internal_set_kernel_policy accepted is ever stored, so waves and bpw are 0 outside mode 2.
inline KernelPolicy policy_fields(int p) { return {p & 0xff, (p >> 8) & 0xff, (p >> 16) & 0xff, (p >> 24) & 1, (p >> 25) & 31}; }
inline KernelPolicy kernel_policy() { return policy_fields(g_kernel_policy.load(std::memory_order_relaxed)); }

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
    if (p.bpw) { sh.bpw = (unsigned)p.bpw; sh.prefetch = (unsigned)p.prefetch; }
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

// the A/B tools' op number (0 unpack, 1 pack, 2 undelta_pack, 3 unpack over a mixed-width column) as the tables know it
struct ToolOp {
    WaveOp wave;
    WindowOp window;
};
inline ToolOp tool_op(int op)
{
    return op == 1 ? ToolOp{WAVE_PACK, WIN_PACK} : op == 2 ? ToolOp{WAVE_UNDELTA_PACK, WIN_UNDELTA_PACK} : ToolOp{WAVE_UNPACK, WIN_UNPACK};
}

// 16 aligned zero bytes stand in for a buffer that has none: the packed side of a mixed-width column whose blocks all have width 0
// (packed_bytes == 0, so any block with a width > 0 fails the kernel's bounds check), the output of a selection that keeps nothing
template <typename T> const T* no_bytes()
{
    static const T zeros[16 / sizeof(T)] __attribute__((aligned(16))) = {0};
    return zeros;
}

// The packed column of a wave-per-block launch: blocks of one `width` back to back, or mixed (widths[] / offsets[] read and checked
// per block by the kernel against packed_bytes).
struct Column {
    bool mixed;
    unsigned width;
    const uint8_t* widths = nullptr;
    const uint64_t* offsets = nullptr;
    size_t packed_bytes = 0;
};
// THE place that fills a WidthsArgs.  refs: FoR's references, null for plain BitPacking -- and for the consumers (fl_consumer_tier.hpp:
// column_args), whose kernels load the references with the block's metadata.  The callers differ in the wave shape, which they state.
template <typename T>
void widths_args(WidthsArgs& a, const Column& col, const void* packed, void* unpacked, const void* refs, size_t ref_stride,
                 uint32_t* err_flag, size_t n_blocks, const WaveShape& sh)
{
    a.packed = static_cast<const char*>(packed);
    a.unpacked = static_cast<char*>(unpacked);
    a.widths = col.mixed ? col.widths : nullptr;
    a.offsets = col.mixed ? col.offsets : nullptr;
    a.err_flag = err_flag;
    a.refs = refs;
    a.ref_stride = ref_stride;
    a.n_blocks = n_blocks;
    a.uniform_width = col.mixed ? 0u : col.width;
    a.packed_bytes = col.mixed ? col.packed_bytes : 0;          // uniform: not read, such calls are validated here, on the host side
    a.bpw = sh.bpw;
    a.prefetch = sh.prefetch;
    a.linear_map = 0;                                           // the A/B tools' own launches set it, never the library's
    a.nt_from = col.mixed ? 0u : fl::nt_read_from(Elem<T>::BITS);   // a mixed-width column always streams
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
        if (packed_bytes == 0 && packed_in && !in) in = no_bytes<T>();
        if (packed_bytes == 0 && packed_out && !out) out = const_cast<T*>(no_bytes<T>());   // never written: every block is skipped or has W = 0
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

// run_chain where the policy chose the pipeline kernel (c.waves); where it did not, or the op has no pipeline form (-1: cannot happen
// today), the cell-column kernel `cell`
template <typename T>
int run_chain_or_stream(int op, WaveChoice c, unsigned w, stream_launch_t cell, const T* in, const T* bases, T* out, size_t n,
                        bool need_in, bool need_out, void* s)
{
    if (c.waves) {
        const int rc = run_chain<T>(op, c.waves, w, in, bases, out, n, s, nullptr, nullptr, 0, nullptr, c.two_blocks);
        if (rc >= 0) return rc;
    }
    return run_stream<T>(cell, in, out, bases, 0, n, need_in, need_out, op != OP_TRANSPOSE && op != OP_UNTRANSPOSE, s);
}

// Uniform-width call served by the wave-per-block kernels (fl_dispatch.hpp decides; 0 waves = cell-column kernel).
template <typename T>
int run_wave_uniform(bool pack, int waves, unsigned w, const T* packed, T* unpacked, const T* refs, size_t ref_stride,
                     size_t n_blocks, void* stream)
{
    if (n_blocks == 0 || (pack && w == 0)) return FL_OK;
    if (!unpacked || (w != 0 && !packed)) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(unpacked)) return FL_ERR_ALIGN;
    const unsigned bpw = uniform_blocks_per_wave(Elem<T>::BITS, pack, w, refs != nullptr);
    const WaveShape sh = with_policy({waves, bpw, bpw > 1});
    WidthsArgs a;
    widths_args<T>(a, {false, w}, packed, unpacked, refs, ref_stride, nullptr, n_blocks, sh);
    return hip_status(widths_launcher<T>(pack)(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// THE path of the seven uniform-width entry points: the width check, the policy's choice (chosen_waves), the wave-per-block kernel, and
// otherwise run_stream on the family's cell-column instance cell.fn[w].  `aux` is FoR's references or Delta's bases.  chain_op < 0:
// BitPacking / FoR on widths_launcher; else Delta's op on the pipeline kernel, which alone may take the table's two-blocks form.
// The order of the checks is each path's own, and the status of a call with two faults depends on it.
template <typename T>
int run_uniform(WaveOp op, int chain_op, const WidthTable<T>& cell, unsigned w, const T* in, const T* aux, size_t aux_stride, T* out,
                size_t n, void* s, bool two_blocks = false)
{
    if (over_width<T>(w)) return FL_ERR_WIDTH;
    const bool pack = op == WAVE_PACK || op == WAVE_FOR_PACK || op == WAVE_TRANSPOSE_DELTA_PACK;
    const bool need_aux = op != WAVE_PACK && op != WAVE_UNPACK;
    const bool need_in = pack || w != 0, need_out = !pack || w != 0;          // the packed side of a W = 0 column has no bytes
    WaveChoice c = chosen_waves(Elem<T>::BITS, w, op);
    if (chain_op >= 0) {
        if (n && misaligned(aux)) return FL_ERR_ALIGN;                         // Delta: the bases' alignment before anything but the width
        c.two_blocks = c.two_blocks && two_blocks;
        return run_chain_or_stream<T>(chain_op, c, w, cell.fn[w], in, aux, out, n, need_in, need_out, s);
    }
    if (c.waves) {
        // before run_wave_uniform's early FL_OK for a W = 0 pack: the unpacked input of a pack and FoR's references are always needed
        if (n && ((pack && !in) || (need_aux && !aux))) return FL_ERR_NULL;
        return pack ? run_wave_uniform<T>(true, c.waves, w, out, const_cast<T*>(in), aux, aux_stride, n, s)
                    : run_wave_uniform<T>(false, c.waves, w, in, out, aux, aux_stride, n, s);
    }
    return run_stream<T>(cell.fn[w], in, out, aux, aux_stride, n, need_in, need_out, need_aux, s);
}

template <typename T> int dev_pack(unsigned w, const T* in, T* out, size_t n, void* s)
{
    return run_uniform<T>(WAVE_PACK, -1, pack_table_impl<T, PACK_PLAIN>(), w, in, nullptr, 0, out, n, s);
}
template <typename T> int dev_unpack(unsigned w, const T* in, T* out, size_t n, void* s)
{
    return run_uniform<T>(WAVE_UNPACK, -1, unpack_table_impl<T, BODY_STORE>(), w, in, nullptr, 0, out, n, s);
}
template <typename T> int dev_for_pack(unsigned w, const T* in, const T* refs, size_t stride, T* out, size_t n, void* s)
{
    return run_uniform<T>(WAVE_FOR_PACK, -1, pack_table_impl<T, PACK_FOR>(), w, in, refs, stride, out, n, s);
}
template <typename T> int dev_unfor_pack(unsigned w, const T* in, const T* refs, size_t stride, T* out, size_t n, void* s)
{
    return run_uniform<T>(WAVE_UNFOR_PACK, -1, unpack_table_impl<T, BODY_ADD_REF>(), w, in, refs, stride, out, n, s);
}
template <typename T> int dev_undelta_pack(unsigned w, const T* in, const T* bases, T* out, size_t n, void* s)
{
    return run_uniform<T>(WAVE_UNDELTA_PACK, OP_UNDELTA_PACK, unpack_table_impl<T, BODY_UNDELTA>(), w, in, bases, 0, out, n, s, true);
}
template <typename T> int dev_undelta_pack_untranspose(unsigned w, const T* in, const T* bases, T* out, size_t n, void* s)
{
    return run_uniform<T>(WAVE_UNDELTA_PACK_UNTRANSPOSE, OP_UNDELTA_PACK_UNTRANSPOSE, unpack_table_impl<T, BODY_UNDELTA_UNTRANSPOSE>(), w, in, bases,
                          0, out, n, s);
}
template <typename T> int dev_transpose_delta_pack(unsigned w, const T* in, const T* bases, T* out, size_t n, void* s)
{
    return run_uniform<T>(WAVE_TRANSPOSE_DELTA_PACK, OP_TRANSPOSE_DELTA_PACK, pack_table_impl<T, PACK_TRANSPOSE_DELTA>(), w, in, bases, 0, out, n, s);
}
// Delta's and Transpose's own bodies have no width: their table row is read at W = T, and the cell-column kernel is per type
template <typename T> int dev_delta(bool inverse, const T* in, const T* bases, T* out, size_t n, void* s)
{
    if (n && misaligned(bases)) return FL_ERR_ALIGN;
    const int waves = chosen_waves(Elem<T>::BITS, Elem<T>::BITS, inverse ? WAVE_UNDELTA : WAVE_DELTA).waves;
    return run_chain_or_stream<T>(inverse ? OP_UNDELTA : OP_DELTA, {waves, false}, Elem<T>::BITS, delta_launcher<T>(inverse), in, bases, out, n, true, true, s);
}
template <typename T> int dev_transpose(bool inverse, const T* in, T* out, size_t n, void* s)
{
    const int waves = chosen_waves(Elem<T>::BITS, Elem<T>::BITS, inverse ? WAVE_UNTRANSPOSE : WAVE_TRANSPOSE).waves;
    return run_chain_or_stream<T>(inverse ? OP_UNTRANSPOSE : OP_TRANSPOSE, {waves, false}, Elem<T>::BITS, transpose_launcher<T>(inverse), in,
                                  static_cast<const T*>(nullptr), out, n, true, true, s);
}
template <typename T>
int dev_unpack_block_sums(unsigned w, const T* in, size_t n, uint64_t* sums, void* s)
{
    if (over_width<T>(w)) return FL_ERR_WIDTH;
    if (n == 0) return FL_OK;
    if (!sums || (w != 0 && !in)) return FL_ERR_NULL;
    if (misaligned(in)) return FL_ERR_ALIGN;
    ReduceArgs a{reinterpret_cast<const u32x4*>(in), sums, nullptr, n};
    return hip_status(sum_table_impl<T>().fn[w](a, static_cast<hipStream_t>(s)));
}
template <typename T>
int dev_unpack_compare(unsigned w, const T* in, int op, T constant, size_t n, uint32_t* mask, void* s)
{
    if (over_width<T>(w)) return FL_ERR_WIDTH;
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
template <typename T>
int dev_unpack_single(unsigned w, const T* packed, size_t n_blocks, const uint64_t* idx, size_t n_idx,
                      T* out, uint32_t* err_flag, void* s)
{
    if (over_width<T>(w)) return FL_ERR_WIDTH;
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
    if (!packed && packed_bytes == 0) packed = no_bytes<T>();      // a column of width-0 blocks has no packed bytes (every lookup is 0)
    if (!widths || !offsets || !idx || !out || !packed) return FL_ERR_NULL;
    SingleArgs a{packed, idx, out, err_flag, n_blocks, n_idx, 0, widths, offsets, packed_bytes};
    return hip_status(unpack_single_launch<T>(a, static_cast<hipStream_t>(s)));
}

// mixed-width columns: device-resident widths[] / offsets[] (fl_widths.hpp)
template <typename T>
int run_widths(bool pack, const uint8_t* widths, const uint64_t* offsets, const void* packed, size_t packed_bytes, void* unpacked,
               size_t n_blocks, uint32_t* err_flag, void* stream, const T* refs = nullptr, size_t ref_stride = 0, bool with_refs = false)
{
    if (n_blocks == 0) return FL_OK;
    if (with_refs && !refs) return FL_ERR_NULL;
    if (!packed && packed_bytes == 0) packed = no_bytes<T>();    // a column whose blocks all have width 0: its packed pointer may be NULL
    if (!widths || !offsets || !packed || !unpacked) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(unpacked)) return FL_ERR_ALIGN;
    const WaveShape sh = with_policy({mixed_waves(Elem<T>::BITS, pack), mixed_blocks_per_wave(Elem<T>::BITS, pack), mixed_prefetch(Elem<T>::BITS)});
    WidthsArgs a;
    widths_args<T>(a, {true, 0, widths, offsets, packed_bytes}, packed, unpacked, with_refs ? refs : nullptr, ref_stride, err_flag, n_blocks, sh);
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

template <typename T> int dev_for_widths(const T* mins, const T* maxs, size_t n, uint8_t* widths, void* s)
{
    if (n == 0) return FL_OK;
    if (!mins || !maxs || !widths) return FL_ERR_NULL;
    return hip_status(launch_for_widths<T>(mins, maxs, n, widths, static_cast<hipStream_t>(s)));
}

// THE place that fills a BatchArgs: many small arrays, device arrays of pointers (fl_batch.hpp).  refs: FoR's; bases: Delta's.
inline void batch_args(BatchArgs& b, const void* const* packed, void* const* unpacked, const uint8_t* widths, const void* refs,
                       const void* const* bases, const uint32_t* n_blocks, size_t n_arrays, uint32_t max_blocks, uint32_t* err_flag,
                       const WaveShape& sh)
{
    b.packed = reinterpret_cast<const char* const*>(packed);
    b.unpacked = reinterpret_cast<char* const*>(unpacked);
    b.widths = widths;
    b.n_blocks = n_blocks;
    b.err_flag = err_flag;
    b.refs = refs;
    b.bases = reinterpret_cast<const char* const*>(bases);
    b.n_arrays = n_arrays;
    b.tiles_per_array = 0;
    b.max_blocks = max_blocks;
    b.bpw = sh.bpw;
    b.prefetch = sh.prefetch;
}

template <typename T>
int run_batch(bool pack, const void* const* packed, void* const* unpacked, const uint8_t* widths, const void* refs, bool with_refs,
              const uint32_t* n_blocks, size_t n_arrays, uint32_t max_blocks, uint32_t* err_flag, void* stream)
{
    if (n_arrays == 0 || max_blocks == 0) return FL_OK;
    if (!packed || !unpacked || !widths || !n_blocks || (with_refs && !refs)) return FL_ERR_NULL;
    if (max_blocks > BATCH_MAX_BLOCKS) return FL_ERR_INDEX;       // 2^30 blocks = 2^40 values in ONE array: a bound nobody means
    const unsigned bpw = batch_blocks_per_wave(Elem<T>::BITS, pack);
    const WaveShape sh = with_policy({batch_waves(Elem<T>::BITS, pack), bpw, bpw > 1});
    BatchArgs b;
    batch_args(b, packed, unpacked, widths, with_refs ? refs : nullptr, nullptr, n_blocks, n_arrays, max_blocks, err_flag, sh);
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
    // one block per wavefront, no prefetch, whatever the policy says: of its overrides the kernel takes the waves alone
    const WaveShape sh{with_policy({mixed_waves(Elem<T>::BITS, op == OP_TRANSPOSE_DELTA_PACK)}).waves, 1, 0};
    BatchArgs b;
    batch_args(b, packed, unpacked, widths, nullptr, bases, n_blocks, n_arrays, max_blocks, err_flag, sh);
    return hip_status(fn(b, max_blocks, sh.waves, static_cast<hipStream_t>(stream)));
}

}  // namespace

// THE list of the element types: M(T, S) once per type and its symbol infix
#define FL_FOR_EACH_TYPE(M) M(uint8_t, u8) M(uint16_t, u16) M(uint32_t, u32) M(uint64_t, u64)

// the consumers of a packed column (unfor_compare ... undelta_compare_range), host side and extern "C", on what is defined above
#include "fl_consumer_tier.hpp"

// ---------------------------------------------------------------------------
// mixed-width columns with the widths kept by the library: device-resident widths[] / offsets[] behind a handle
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
int run_mixed(bool pack, const fl_mixed_plan* p, const void* packed, void* unpacked, void* stream)
{
    if (!p) return FL_ERR_NULL;
    if (p->type_bits != (unsigned)Elem<T>::BITS) return FL_ERR_WIDTH;
    if (p->n_blocks == 0) return FL_OK;
    if (!unpacked || (p->packed_bytes && !packed)) return FL_ERR_NULL;
    // widths were validated at plan creation; an all-zero-width column has no packed bytes at all (run_widths accepts NULL then)
    return run_widths<T>(pack, p->d_widths, p->d_offsets, p->packed_bytes ? packed : nullptr, p->packed_bytes, unpacked, p->n_blocks, nullptr, stream);
}

// the A/B tools' timed call (fl_internal_selftune_check): what the public entry point of (T, op) does
template <typename T>
int selftune_call(int op, unsigned w, const void* in, const void* aux, void* out, size_t n, void* s)
{
    if (op == 2) {
        FL_DEVICE_TIER(s, in, aux, out);
        return dev_undelta_pack<T>(w, static_cast<const T*>(in), static_cast<const T*>(aux), static_cast<T*>(out), n, s);
    }
    FL_DEVICE_TIER(s, in, out);
    return op == 1 ? dev_pack<T>(w, static_cast<const T*>(in), static_cast<T*>(out), n, s)
                   : dev_unpack<T>(w, static_cast<const T*>(in), static_cast<T*>(out), n, s);
}

}  // namespace

extern "C" {

int fl_widths_to_offsets(unsigned type_bits, const uint8_t* widths, size_t n_blocks, uint64_t* offsets,
                         uint64_t* total_bytes, uint32_t* err_flag, void* stream)
{
    if (!valid_type_bits(type_bits)) return FL_ERR_WIDTH;
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

void fl_mixed_plan_destroy(fl_mixed_plan* p)
{
    if (!p) return;
    if (p->d_widths) (void)hipFree(p->d_widths);
    if (p->d_offsets) (void)hipFree(p->d_offsets);
    delete p;
}
int fl_mixed_plan_create(unsigned type_bits, const uint8_t* widths, size_t n_blocks, fl_mixed_plan** plan)
{
    if (!plan || (n_blocks && !widths)) return FL_ERR_NULL;
    *plan = nullptr;
    if (!valid_type_bits(type_bits)) return FL_ERR_WIDTH;
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

size_t fl_mixed_plan_n_blocks(const fl_mixed_plan* p) { return p ? p->n_blocks : 0; }
uint64_t fl_mixed_plan_packed_bytes(const fl_mixed_plan* p) { return p ? p->packed_bytes : 0; }
const uint64_t* fl_mixed_plan_offsets(const fl_mixed_plan* p) { return p ? p->d_offsets : nullptr; }
const uint8_t* fl_mixed_plan_widths(const fl_mixed_plan* p) { return p ? p->d_widths : nullptr; }

int fl_fill_random(void* dst, size_t n_bytes, uint64_t seed, void* stream)
{
    if (n_bytes == 0) return FL_OK;
    if (!dst) return FL_ERR_NULL;
    if ((reinterpret_cast<uintptr_t>(dst) & 7u) || (n_bytes & 7u)) return FL_ERR_ALIGN;
    FL_DEVICE_TIER(stream, dst);
    return hip_status(launch_fill_random(static_cast<uint64_t*>(dst), n_bytes / 8, seed, static_cast<hipStream_t>(stream)));
}

void fl_host_release(void) { g_host.release(); }

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
    if (!valid_type_bits(type_bits)) return 0;
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
        if (over_width<T>(w)) return FL_ERR_WIDTH;                                                        \
        return host_run<T>(in, n * 1024, nullptr, 0, out, n * plen<T>(w),                                 \
                           [&](const T* di, const T*, T* d_o, void* st) { return dev_pack<T>(w, di, d_o, n, st); }); \
    }                                                                                                     \
    int fl_##S##_unpack_host(unsigned w, const T* in, T* out, size_t n)                                   \
    {                                                                                                     \
        if (over_width<T>(w)) return FL_ERR_WIDTH;                                                        \
        return host_run<T>(in, n * plen<T>(w), nullptr, 0, out, n * 1024,                                 \
                           [&](const T* di, const T*, T* d_o, void* st) { return dev_unpack<T>(w, di, d_o, n, st); }); \
    }                                                                                                     \
    int fl_##S##_unpack_single_host(unsigned w, const T* pk, size_t n, uint64_t index, T* value)          \
    { return host_unpack_single<T>(w, pk, n, index, value); }                                             \
    int fl_##S##_for_pack_host(unsigned w, const T* in, T reference, T* out, size_t n)                    \
    {                                                                                                     \
        if (over_width<T>(w)) return FL_ERR_WIDTH;                                                        \
        return host_run<T>(in, n * 1024, &reference, 1, out, n * plen<T>(w),                              \
                           [&](const T* di, const T* da, T* d_o, void* st) { return dev_for_pack<T>(w, di, da, 0, d_o, n, st); }); \
    }                                                                                                     \
    int fl_##S##_unfor_pack_host(unsigned w, const T* in, T reference, T* out, size_t n)                  \
    {                                                                                                     \
        if (over_width<T>(w)) return FL_ERR_WIDTH;                                                        \
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
        if (over_width<T>(w)) return FL_ERR_WIDTH;                                                        \
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

FL_FOR_EACH_TYPE(FL_DEFINE_TYPE)


// ---- fl_internal_*: the hooks of the tests and the A/B tools (include/fastlanes_amd_internal.h), not part of the stable ABI ----------
void fl_internal_set_kernel_policy(int policy)
{
    const KernelPolicy p = policy_fields(policy);
    const bool ok = policy >= 0 && policy < (1 << 30) && p.mode <= 2 && (p.waves == 0 || (p.waves >= 3 && p.waves <= 8)) && p.bpw <= 16
                    && (p.mode == 2 || (p.waves == 0 && p.bpw == 0)) && (p.prefetch == 0 || p.bpw >= 2) && (p.window == 0 || p.window >= 8);
    g_kernel_policy.store(ok ? policy : 0, std::memory_order_relaxed);
    fl::window_override().store(ok ? p.window : 0, std::memory_order_relaxed);
}
int fl_internal_get_kernel_policy(void) { return g_kernel_policy.load(std::memory_order_relaxed); }
uint64_t fl_internal_zero_copy_fallbacks(void) { return g_zero_copy_fallbacks.load(std::memory_order_relaxed); }

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
    if (!valid_type_bits(type_bits)) return FL_ERR_INDEX;
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
    // two blocks per wavefront: same bytes per launch, the occupancy is what the table says
    int w = op == 3 ? mixed_waves(type_bits, false) : chosen_waves(type_bits, width, tool_op(op).wave).waves;
    if (w == 0) w = 8;       // a cell-column kernel gives a wavefront 8 blocks at 2-3 waves per SIMD: the one-unit-per-wavefront stream needs every slot to keep as many bytes in flight
    *waves = w < 3 ? 3 : w;
    *nt_loads = op == 1 || op == 3 || width >= fl::nt_read_from(type_bits);       // fl_widths.hpp: RD_AUTO; pack reads non-temporally
    *window_log2_units = window_log2_blocks(tool_op(op).window, type_bits);
    return FL_OK;
}

int fl_internal_selftune_check(int op, unsigned type_bits, unsigned width, const void* in, const void* aux, void* out, size_t n_blocks, void* stream,
                               float* table_ms, float* best_other_ms, int* best_other_policy)
{
    if (!table_ms || !best_other_ms || !best_other_policy) return FL_ERR_NULL;
    if (op < 0 || op > 2 || !valid_type_bits(type_bits)) return FL_ERR_INDEX;
    if (width > type_bits) return FL_ERR_WIDTH;
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto call = [&]() -> int {
        return type_bits == 8 ? selftune_call<uint8_t>(op, width, in, aux, out, n_blocks, stream)
             : type_bits == 16 ? selftune_call<uint16_t>(op, width, in, aux, out, n_blocks, stream)
             : type_bits == 32 ? selftune_call<uint32_t>(op, width, in, aux, out, n_blocks, stream)
                               : selftune_call<uint64_t>(op, width, in, aux, out, n_blocks, stream);
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
    const fl::WaveOp wop = tool_op(op).wave;
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

}  // extern "C"
