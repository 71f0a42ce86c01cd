// fl_capi.hip -- the extern "C" boundary declared in include/fastlanes_amd.h.
// Validates arguments, maps the runtime width to the per-(T,W) kernel instance
// (the reference's `match width`, bitpacking.rs:82-95) and launches it.  No CPU
// compute path exists in this library: every entry point ends in a HIP launch.
// In this order: the kernel policy; the builders of the launch-argument blocks and the device tier's validators (run_* / dev_*);
// fl_mixed_plan; extern "C" -- the public entry points, then the fl_internal_* ones of the A/B tools.  The host tier (HostCtx, host_run)
// is fl_host_tier.hpp, part of this translation unit; fl_column_pair_alloc / _free and the memory-class probe live in fl_pair.hip.
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
#include "fl_for_compare_in.hpp"
#include "fl_aggregate_by_columns.hpp"
#include "fl_set_build.hpp"
#include "fl_lookup.hpp"
#include "fl_aggregate_by_lookup.hpp"
#include "fl_delta_compare_range.hpp"
#include "fl_aggregate_by_window.hpp"
#include "fl_select.hpp"
#include "fl_aggregate.hpp"
#include "fl_aggregate_by.hpp"
#include "fl_for_compare_columns.hpp"
#include "fl_aggregate_columns.hpp"
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
// THE place that fills a WidthsArgs.  refs: FoR's references, null for plain BitPacking -- and for the four consumers, whose kernels
// load the references with the block's metadata.  The callers differ in the wave shape, which they state.
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

// The consumers of a FoR-packed column (fl_for_block.hpp): unfor_compare, unfor_compare_range, unfor_select, unfor_aggregate (and
// unfor_aggregate_by, which takes two of them), each over
// a uniform-width column (col.width, blocks back to back) or a mixed-width one (widths[] / offsets[], checked per block by the kernel).
// false: one of the column's pointers is missing (FL_ERR_NULL).  A mixed-width column whose blocks all have width 0 has no packed bytes:
// its packed pointer may be NULL (run_widths) and is replaced here.
template <typename T> bool block_consumer_column(const Column& col, const T*& packed, const T* refs)
{
    if (col.mixed && !packed && col.packed_bytes == 0) packed = no_bytes<T>();
    return refs && (!col.mixed || (col.widths && col.offsets)) && (packed || (!col.mixed && col.width == 0));
}
// the WidthsArgs part of the four argument blocks, launched with the shape of unfor_pack_widths: the same blocks, the same reads
template <typename T>
WaveShape block_consumer_args(WidthsArgs& a, const Column& col, const T* packed, size_t ref_stride, size_t n_blocks, uint32_t* err_flag)
{
    const WaveShape sh = with_policy({mixed_waves(Elem<T>::BITS, false), mixed_blocks_per_wave(Elem<T>::BITS, false), mixed_prefetch(Elem<T>::BITS)});
    widths_args<T>(a, col, packed, nullptr, nullptr, ref_stride, err_flag, n_blocks, sh);
    return sh;
}

// unfor_compare (fl_for_compare.hpp).  The predicate becomes its cyclic interval here, once per call.
template <typename T>
int run_unfor_compare(const Column& col, const T* packed, const T* refs, size_t ref_stride, int op, T constant, size_t n_blocks,
                      uint32_t* mask, uint32_t* err_flag, void* stream)
{
    if (!col.mixed && over_width<T>(col.width)) return FL_ERR_WIDTH;
    if (op < FL_CMP_EQ || op > FL_CMP_GE) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (!block_consumer_column(col, packed, refs) || !mask) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(mask)) return FL_ERR_ALIGN;
    const ForPredicate p = for_compare_predicate(Elem<T>::BITS, op, constant);
    ForCompareArgs a;
    const WaveShape sh = block_consumer_args<T>(a, col, packed, ref_stride, n_blocks, col.mixed ? err_flag : nullptr);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = refs;
    a.cmp_a = p.a;
    a.cmp_s = p.s;
    a.cmp_none = p.none ? 1u : 0u;
    return hip_status(for_compare_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_compare_range: run_unfor_compare with the cyclic interval [lo, hi] as the predicate and the mask so far beside it
// (fl_for_compare_range.hpp).  The same launch shape, the same checks in the same order; `mask` may be `mask_in`.
template <typename T>
int run_unfor_compare_range(const Column& col, const T* packed, const T* refs, size_t ref_stride, T lo, T hi, int combine,
                            const uint32_t* mask_in, size_t n_blocks, uint32_t* mask, uint32_t* err_flag, void* stream)
{
    if (!col.mixed && over_width<T>(col.width)) return FL_ERR_WIDTH;
    if (combine < FL_MASK_NEW || combine > FL_MASK_OR) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (combine == FL_MASK_NEW) mask_in = nullptr;                       // ignored: never read, never checked
    else if (!mask_in) return FL_ERR_NULL;
    if (!block_consumer_column(col, packed, refs) || !mask) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(mask) || misaligned(mask_in)) return FL_ERR_ALIGN;
    const ForPredicate p = for_range_predicate(Elem<T>::BITS, lo, hi);
    ForRangeArgs a;
    const WaveShape sh = block_consumer_args<T>(a, col, packed, ref_stride, n_blocks, col.mixed ? err_flag : nullptr);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = refs;
    a.cmp_a = p.a;
    a.cmp_s = p.s;
    a.cmp_none = 0u;
    a.mask_in = reinterpret_cast<const char*>(mask_in);
    a.combine = (unsigned)combine;
    return hip_status(for_range_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// undelta_compare_range (fl_delta_compare_range.hpp): run_unfor_compare_range over a Delta-packed column -- `bases` (LANES per block, 128
// bytes, read as 16-byte cells) stands where the references stood.  The same checks in the same order, `bases` among the required and
// the aligned pointers; one block per wavefront for every type, at unfor_pack_widths' occupancy; `mask` may be `mask_in`.
template <typename T>
int run_undelta_compare_range(const Column& col, const T* packed, const T* bases, T lo, T hi, int combine, const uint32_t* mask_in,
                              size_t n_blocks, uint32_t* mask, uint32_t* err_flag, void* stream)
{
    if (!col.mixed && over_width<T>(col.width)) return FL_ERR_WIDTH;
    if (combine < FL_MASK_NEW || combine > FL_MASK_OR) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (combine == FL_MASK_NEW) mask_in = nullptr;                       // ignored: never read, never checked
    else if (!mask_in) return FL_ERR_NULL;
    if (!block_consumer_column(col, packed, bases) || !mask) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(bases) || misaligned(mask) || misaligned(mask_in)) return FL_ERR_ALIGN;
    const ForPredicate p = for_range_predicate(Elem<T>::BITS, lo, hi);
    const WaveShape sh = with_policy({mixed_waves(Elem<T>::BITS, false), 1u, 0u});
    DeltaRangeArgs a;
    widths_args<T>(a, col, packed, nullptr, nullptr, 0, col.mixed ? err_flag : nullptr, n_blocks, sh);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = nullptr;
    a.cmp_a = p.a;
    a.cmp_s = p.s;
    a.cmp_none = 0u;
    a.mask_in = reinterpret_cast<const char*>(mask_in);
    a.combine = (unsigned)combine;
    a.bases = reinterpret_cast<const char*>(bases);
    return hip_status(delta_range_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_compare_in: run_unfor_compare_range with the member set's window as the predicate and its bitmap beside it
// (fl_for_compare_in.hpp, fl_set_decide.hpp).  The same launch shape, the same checks in the same order, the set's own among them:
// negate and set_bits with combine (FL_ERR_INDEX), set_words with the other pointers (FL_ERR_NULL, FL_ERR_ALIGN; never read when
// set_bits == 0).  set_bits decides the tier here, once per call: up to SET_REGISTER_BITS the bitmap rides in a VGPR.
template <typename T>
int run_unfor_compare_in(const Column& col, const T* packed, const T* refs, size_t ref_stride, T set_lo, uint64_t set_bits,
                         const uint32_t* set_words, int negate, int combine, const uint32_t* mask_in, size_t n_blocks, uint32_t* mask,
                         uint32_t* err_flag, void* stream)
{
    if (!col.mixed && over_width<T>(col.width)) return FL_ERR_WIDTH;
    if (combine < FL_MASK_NEW || combine > FL_MASK_OR || negate < 0 || negate > 1 || set_bits > set_max_bits(Elem<T>::BITS)) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (combine == FL_MASK_NEW) mask_in = nullptr;                       // ignored: never read, never checked
    else if (!mask_in) return FL_ERR_NULL;
    if (set_bits == 0) set_words = nullptr;                              // the empty set: never read, never checked
    else if (!set_words) return FL_ERR_NULL;
    if (!block_consumer_column(col, packed, refs) || !mask) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(mask) || misaligned(mask_in) || misaligned(set_words)) return FL_ERR_ALIGN;
    const ForPredicate p = set_window(Elem<T>::BITS, set_lo, set_bits);
    ForInArgs a;
    const WaveShape sh = block_consumer_args<T>(a, col, packed, ref_stride, n_blocks, col.mixed ? err_flag : nullptr);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = refs;
    a.cmp_a = p.a;
    a.cmp_s = p.s;
    a.cmp_none = p.none ? 1u : 0u;
    a.mask_in = reinterpret_cast<const char*>(mask_in);
    a.combine = (unsigned)combine;
    a.set_words = set_words;
    a.set_bytes = (unsigned)(4u * set_word_count(set_bits));
    a.negate = (unsigned)negate;
    return hip_status(for_in_launcher<T>(set_bits <= SET_REGISTER_BITS)(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_set_build (fl_set_build.hpp): the member set unfor_compare_in probes, built from a column under a mask.  The window's checks are
// run_unfor_compare_in's, in its order: the width; set_bits (FL_ERR_INDEX); the empty column; set_words (never touched when set_bits
// == 0) and the column's pointers (FL_ERR_NULL); alignment, set_words and stats included.  `mask` and `stats` may be NULL.  set_bits
// decides the tier here, once per call (fl_set_build_map.hpp: set_build_lds_tier).  The memory tier ships SET_BUILD_MEMORY_TIER; the
// timing tool measures the other variant beside it through the environment variable FL_INTERNAL_SET_BUILD_VARIANT (1: one atomic per
// element, 2: test before set; read on every memory-tier call, bits identical either way).  The persistent grid takes the policy's
// waves and blocks per wavefront as run_unfor_aggregate_by does.
constexpr int SET_BUILD_MEMORY_TIER = SETB_MEM_TEST;
inline int set_build_tier(uint64_t set_bits)
{
    if (set_build_lds_tier(set_bits)) return SETB_LDS;
    if (const char* v = std::getenv("FL_INTERNAL_SET_BUILD_VARIANT")) {
        if (v[0] == '1' && !v[1]) return SETB_MEM;
        if (v[0] == '2' && !v[1]) return SETB_MEM_TEST;
    }
    return SET_BUILD_MEMORY_TIER;
}
template <typename T>
int run_unfor_set_build(const Column& col, const T* packed, const T* refs, size_t ref_stride, const uint32_t* mask, size_t n_blocks, T set_lo,
                        uint64_t set_bits, uint32_t* set_words, uint64_t* stats, uint32_t* err_flag, void* stream)
{
    if (!col.mixed && over_width<T>(col.width)) return FL_ERR_WIDTH;
    if (set_bits > set_max_bits(Elem<T>::BITS)) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (set_bits == 0) set_words = nullptr;                              // the empty window: never touched, never checked
    else if (!set_words) return FL_ERR_NULL;
    if (!block_consumer_column(col, packed, refs)) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(mask) || misaligned(set_words) || misaligned(stats)) return FL_ERR_ALIGN;
    const ForPredicate p = set_window(Elem<T>::BITS, set_lo, set_bits);
    const WaveShape sh = with_policy({0, 0u, 0u});
    SetBuildArgs a;
    widths_args<T>(a.col, col, packed, nullptr, nullptr, ref_stride, col.mixed ? err_flag : nullptr, n_blocks, sh);
    a.refs = refs;
    a.mask = mask;
    a.set_words = set_words;
    a.stats = stats;
    a.cmp_a = p.a;
    a.cmp_s = p.s;
    a.cmp_none = p.none ? 1u : 0u;
    a.n_words = (unsigned)set_word_count(set_bits);
    a.last_mask = set_build_last_word_mask(set_bits);
    a.run = 0;
    const set_build_launch_t fn = set_build_launcher<T>(set_build_tier(set_bits));
    if (!fn) return hip_fail(hipErrorInvalidDeviceFunction);
    return hip_status(fn(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_aggregate_by_window (fl_aggregate_by_window.hpp): a value column and a key column of T of the same form, both uniform or both
// mixed, grouped inside the window [key_lo, key_lo + n_groups - 1] into the caller's four arrays.  One validator, one builder.
// The validator's order is run_unfor_set_build's: the widths; n_groups (FL_ERR_INDEX); the empty column; the columns' pointers
// (FL_ERR_NULL; the four arrays, `mask` and `stats` may be NULL); alignment, the arrays and stats included.  An empty window touches no
// array: the builder drops them, so they are neither maintained nor checked.
struct WindowArrays {
    uint64_t *counts, *sums, *mins, *maxs, *stats;
};
template <typename T>
int aggregate_by_window_refusal(const Column& col, const T*& packed, const T* refs, const Column& kcol, const T*& keys, const T* key_refs,
                                const uint32_t* mask, size_t n_blocks, uint64_t n_groups, WindowArrays& t)
{
    if ((!col.mixed && over_width<T>(col.width)) || (!kcol.mixed && over_width<T>(kcol.width))) return FL_ERR_WIDTH;
    if (n_groups > aggregate_by_window_max_groups(Elem<T>::BITS)) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (n_groups == 0) t.counts = t.sums = t.mins = t.maxs = nullptr;    // the empty window: never touched, never checked
    if (!block_consumer_column(col, packed, refs) || !block_consumer_column(kcol, keys, key_refs)) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(keys) || misaligned(mask) || misaligned(t.counts) || misaligned(t.sums) || misaligned(t.mins) ||
        misaligned(t.maxs) || misaligned(t.stats))
        return FL_ERR_ALIGN;
    return FL_OK;
}
template <typename T>
AggregateByWindowArgs aggregate_by_window_args(const Column& col, const T* packed, const T* refs, size_t ref_stride, const Column& kcol, const T* keys,
                                               const T* key_refs, size_t key_ref_stride, const uint32_t* mask, size_t n_blocks, T key_lo,
                                               uint64_t n_groups, const WindowArrays& t, uint32_t* err_flag, const WaveShape& sh)
{
    const ForPredicate p = set_window(Elem<T>::BITS, key_lo, n_groups);
    AggregateByWindowArgs a;
    widths_args<T>(a.val, col, packed, nullptr, nullptr, ref_stride, col.mixed ? err_flag : nullptr, n_blocks, sh);
    widths_args<T>(a.key, kcol, keys, nullptr, nullptr, key_ref_stride, col.mixed ? err_flag : nullptr, n_blocks, sh);
    a.val_refs = refs;
    a.key_refs = key_refs;
    a.mask = mask;
    a.counts = t.counts;
    a.sums = t.sums;
    a.mins = t.mins;
    a.maxs = t.maxs;
    a.stats = t.stats;
    a.cmp_a = p.a;
    a.cmp_s = p.s;
    a.cmp_none = p.none ? 1u : 0u;
    a.need_values = t.sums || t.mins || t.maxs ? 1u : 0u;
    a.n_slots = aggregate_by_window_lds_tier(n_groups) ? (unsigned)n_groups : 0u;
    a.run = 0;
    return a;
}
template <typename T>
int run_unfor_aggregate_by_window(const Column& col, const T* packed, const T* refs, size_t ref_stride, const Column& kcol, const T* keys,
                                  const T* key_refs, size_t key_ref_stride, const uint32_t* mask, size_t n_blocks, T key_lo, uint64_t n_groups,
                                  WindowArrays t, uint32_t* err_flag, void* stream)
{
    if (const int rc = aggregate_by_window_refusal<T>(col, packed, refs, kcol, keys, key_refs, mask, n_blocks, n_groups, t); rc != FL_OK || n_blocks == 0)
        return rc;
    const WaveShape sh = with_policy({0, 0u, 0u});
    const AggregateByWindowArgs a =
        aggregate_by_window_args<T>(col, packed, refs, ref_stride, kcol, keys, key_refs, key_ref_stride, mask, n_blocks, key_lo, n_groups, t, err_flag, sh);
    const aggregate_by_window_launch_t fn = aggregate_by_window_launcher<T>(aggregate_by_window_lds_tier(n_groups) ? AGGW_LDS : AGGW_MEM);
    if (!fn) return hip_fail(hipErrorInvalidDeviceFunction);
    return hip_status(fn(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_lookup (fl_lookup.hpp): table[(key - key_lo) mod 2^T] of every kept row of a key column, U = T or uint8_t, written in full-width
// packed order with the hits as a mask beside it.  One validator, one builder.  The validator's order is run_unfor_set_build's: the
// width; n_slots (FL_ERR_INDEX: above min(2^T, 2^32) slots, or a table of 2^31 bytes or more); the empty column; `table` (never read
// when n_slots == 0), `out` and the column's pointers (FL_ERR_NULL; `mask`, `present`, `hit_mask` and `stats` may be NULL); alignment.
// An empty window reads neither the table nor the bitmap: the validator drops them, so they are neither read nor checked.  n_slots
// decides the tier here, once per call (fl_lookup_map.hpp: lookup_tier).  The persistent grid takes the policy's waves and blocks per
// wavefront as run_unfor_set_build does.
struct LookupTable {
    const void* table;
    const uint32_t* present;
    uint64_t missing;
    void* out;
    uint32_t* hit_mask;
    uint64_t* stats;
};
template <typename T>
int lookup_refusal(const Column& col, const T*& packed, const T* refs, const uint32_t* mask, size_t n_blocks, uint64_t n_slots, unsigned payload_bytes,
                   LookupTable& t)
{
    if (!col.mixed && over_width<T>(col.width)) return FL_ERR_WIDTH;
    if (lookup_slots_refused(Elem<T>::BITS, n_slots, payload_bytes)) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (n_slots == 0) t.table = t.present = nullptr;                      // the empty window: never read, never checked
    else if (!t.table) return FL_ERR_NULL;
    if (!block_consumer_column(col, packed, refs) || !t.out) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(mask) || misaligned(t.hit_mask) || misaligned(t.present) || misaligned(t.table) || misaligned(t.out) ||
        misaligned(t.stats))
        return FL_ERR_ALIGN;
    return FL_OK;
}
template <typename T>
LookupArgs lookup_args(const Column& col, const T* packed, const T* refs, size_t ref_stride, const uint32_t* mask, size_t n_blocks, T key_lo,
                       uint64_t n_slots, unsigned payload_bytes, const LookupTable& t, uint32_t* err_flag, const WaveShape& sh)
{
    const ForPredicate p = set_window(Elem<T>::BITS, key_lo, n_slots);
    LookupArgs a;
    widths_args<T>(a.col, col, packed, nullptr, nullptr, ref_stride, col.mixed ? err_flag : nullptr, n_blocks, sh);
    a.refs = refs;
    a.mask = mask;
    a.table = t.table;
    a.present = t.present;
    a.out = static_cast<char*>(t.out);
    a.hit_mask = t.hit_mask;
    a.stats = t.stats;
    a.cmp_a = p.a;
    a.cmp_s = p.s;
    a.missing = t.missing;
    a.cmp_none = p.none ? 1u : 0u;
    a.table_bytes = (unsigned)(n_slots * payload_bytes);
    a.present_bytes = t.present ? (unsigned)(4u * set_word_count(n_slots)) : 0u;
    a.run = 0;
    return a;
}
template <typename T>
int run_unfor_lookup(const Column& col, const T* packed, const T* refs, size_t ref_stride, const uint32_t* mask, size_t n_blocks, T key_lo,
                     uint64_t n_slots, unsigned payload_bytes, LookupTable t, uint32_t* err_flag, void* stream)
{
    if (const int rc = lookup_refusal<T>(col, packed, refs, mask, n_blocks, n_slots, payload_bytes, t); rc != FL_OK || n_blocks == 0) return rc;
    const WaveShape sh = with_policy({0, 0u, 0u});
    const LookupArgs a = lookup_args<T>(col, packed, refs, ref_stride, mask, n_blocks, key_lo, n_slots, payload_bytes, t, err_flag, sh);
    const lookup_launch_t fn = lookup_launcher<T>(payload_bytes, lookup_tier(n_slots, payload_bytes));
    if (!fn) return hip_fail(hipErrorInvalidDeviceFunction);
    return hip_status(fn(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_aggregate_by_lookup (fl_aggregate_by_lookup.hpp): unfor_lookup_u8 and unfor_aggregate_by in one pass -- a value column and a key
// column of T of the same form, both uniform or both mixed, a u8 table over the window [key_lo, key_lo + n_slots - 1], 256 groups.  One
// validator, one builder.  The validator's order is that of the two parents: the widths; n_slots (FL_ERR_INDEX, lookup_slots_refused with
// a one-byte payload); `result` (written by EVERY call -- the init launch also answers an empty column -- so it is required before the
// empty-column return), `table` (never read when n_slots == 0: the validator drops it and `present`, so they are neither read nor
// checked) and the columns' pointers (FL_ERR_NULL; `mask`, `present` and `stats` may be NULL); alignment.  The persistent grid takes
// the policy's waves and blocks per wavefront as run_unfor_aggregate_by does.
struct LookupGroups {
    const uint8_t* table;
    const uint32_t* present;
    void* result;
    uint64_t* stats;
};
template <typename T>
int aggregate_by_lookup_refusal(const Column& col, const T*& packed, const T* refs, const Column& kcol, const T*& keys, const T* key_refs,
                                const uint32_t* mask, size_t n_blocks, uint64_t n_slots, LookupGroups& t)
{
    if ((!col.mixed && over_width<T>(col.width)) || (!kcol.mixed && over_width<T>(kcol.width))) return FL_ERR_WIDTH;
    if (lookup_slots_refused(Elem<T>::BITS, n_slots, 1u)) return FL_ERR_INDEX;
    if (!t.result) return FL_ERR_NULL;
    if (n_blocks) {
        if (n_slots == 0) {                                              // the empty window: never read, never checked
            t.table = nullptr;
            t.present = nullptr;
        } else if (!t.table) {
            return FL_ERR_NULL;
        }
        if (!block_consumer_column(col, packed, refs) || !block_consumer_column(kcol, keys, key_refs)) return FL_ERR_NULL;
        if (misaligned(packed) || misaligned(keys) || misaligned(mask) || misaligned(t.present) || misaligned(t.table) || misaligned(t.stats))
            return FL_ERR_ALIGN;
    }
    return misaligned(t.result) ? FL_ERR_ALIGN : FL_OK;
}
template <typename T>
AggregateByLookupArgs aggregate_by_lookup_args(const Column& col, const T* packed, const T* refs, size_t ref_stride, const Column& kcol, const T* keys,
                                               const T* key_refs, size_t key_ref_stride, const uint32_t* mask, size_t n_blocks, T key_lo,
                                               uint64_t n_slots, const LookupGroups& t, uint32_t* err_flag, const WaveShape& sh)
{
    const ForPredicate p = set_window(Elem<T>::BITS, key_lo, n_slots);
    AggregateByLookupArgs a;
    widths_args<T>(a.val, col, packed, nullptr, nullptr, ref_stride, col.mixed ? err_flag : nullptr, n_blocks, sh);
    widths_args<T>(a.key, kcol, keys, nullptr, nullptr, key_ref_stride, col.mixed ? err_flag : nullptr, n_blocks, sh);
    a.val_refs = refs;
    a.key_refs = key_refs;
    a.mask = mask;
    a.table = t.table;
    a.present = t.present;
    a.result = static_cast<BlockAggregate*>(t.result);
    a.stats = t.stats;
    a.cmp_a = p.a;
    a.cmp_s = p.s;
    a.cmp_none = p.none ? 1u : 0u;
    a.table_bytes = (unsigned)n_slots;
    a.present_bytes = t.present ? (unsigned)(4u * set_word_count(n_slots)) : 0u;
    a.run = 0;
    return a;
}
template <typename T>
int run_unfor_aggregate_by_lookup(const Column& col, const T* packed, const T* refs, size_t ref_stride, const Column& kcol, const T* keys,
                                  const T* key_refs, size_t key_ref_stride, const uint32_t* mask, size_t n_blocks, T key_lo, uint64_t n_slots,
                                  LookupGroups t, uint32_t* err_flag, void* stream)
{
    if (const int rc = aggregate_by_lookup_refusal<T>(col, packed, refs, kcol, keys, key_refs, mask, n_blocks, n_slots, t); rc != FL_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipError_t e = launch_aggregate_by_init(static_cast<BlockAggregate*>(t.result), s); e != hipSuccess || n_blocks == 0) return hip_status(e);
    const WaveShape sh = with_policy({0, 0u, 0u});
    const AggregateByLookupArgs a =
        aggregate_by_lookup_args<T>(col, packed, refs, ref_stride, kcol, keys, key_refs, key_ref_stride, mask, n_blocks, key_lo, n_slots, t, err_flag, sh);
    return hip_status(aggregate_by_lookup_launcher<T>()(a, sh.waves, s));
}

// unfor_compare_columns (fl_for_compare_columns.hpp): two columns of T of the same form, both uniform or both mixed.  The six ops become
// one base relation, "swap the columns" and "invert" here, once per call (fl_columns_decide.hpp: columns_relation); the swap is done
// here, so the kernel's column a is always the base relation's left side.  The launch shape and the order of the checks are those of
// run_unfor_compare_range; `mask` may be `mask_in`.
template <typename T>
int run_unfor_compare_columns(const Column& cola, const T* a_packed, const T* a_refs, size_t a_ref_stride, const Column& colb, const T* b_packed,
                              const T* b_refs, size_t b_ref_stride, int op, int is_signed, int combine, const uint32_t* mask_in,
                              size_t n_blocks, uint32_t* mask, uint32_t* err_flag, void* stream)
{
    if ((!cola.mixed && over_width<T>(cola.width)) || (!colb.mixed && over_width<T>(colb.width))) return FL_ERR_WIDTH;
    if (op < FL_CMP_EQ || op > FL_CMP_GE || combine < FL_MASK_NEW || combine > FL_MASK_OR) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (combine == FL_MASK_NEW) mask_in = nullptr;                       // ignored: never read, never checked
    else if (!mask_in) return FL_ERR_NULL;
    if (!block_consumer_column(cola, a_packed, a_refs) || !block_consumer_column(colb, b_packed, b_refs) || !mask) return FL_ERR_NULL;
    if (misaligned(a_packed) || misaligned(b_packed) || misaligned(mask) || misaligned(mask_in)) return FL_ERR_ALIGN;
    const ColumnsRelation rel = columns_relation(op);
    ForColumnsArgs a;
    uint32_t* ef = cola.mixed ? err_flag : nullptr;
    const WaveShape sh = rel.swap ? block_consumer_args<T>(a, colb, b_packed, b_ref_stride, n_blocks, ef)
                                  : block_consumer_args<T>(a, cola, a_packed, a_ref_stride, n_blocks, ef);
    if (rel.swap) block_consumer_args<T>(a.b, cola, a_packed, a_ref_stride, n_blocks, ef);
    else block_consumer_args<T>(a.b, colb, b_packed, b_ref_stride, n_blocks, ef);
    a.mask = reinterpret_cast<char*>(mask);
    a.cmp_refs = rel.swap ? b_refs : a_refs;
    a.b_refs = rel.swap ? a_refs : b_refs;
    a.cmp_a = a.cmp_s = 0;
    a.cmp_none = 0u;
    a.mask_in = reinterpret_cast<const char*>(mask_in);
    a.combine = (unsigned)combine;
    a.bias = columns_bias(Elem<T>::BITS, is_signed != 0);
    a.is_eq = rel.is_eq ? 1u : 0u;
    a.invert = rel.invert ? 1u : 0u;
    return hip_status(for_columns_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_select (fl_select.hpp).  Launched with the shape of unfor_pack_widths, as unfor_compare is.
template <typename T>
int run_unfor_select(const Column& col, const T* packed, const T* refs, size_t ref_stride, const uint32_t* mask, const uint64_t* out_offsets,
                     T* out, size_t out_len, size_t n_blocks, uint32_t* err_flag, void* stream)
{
    if (!col.mixed && over_width<T>(col.width)) return FL_ERR_WIDTH;
    if (n_blocks == 0) return FL_OK;
    // a selection that keeps nothing has no output: `out` may be NULL with out_len == 0 (a non-empty block then fails the kernel's
    // bounds check; nothing is ever written through this pointer)
    if (!out && out_len == 0) out = const_cast<T*>(no_bytes<T>());
    if (!block_consumer_column(col, packed, refs) || !mask || !out_offsets || !out) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(mask) || misaligned(out)) return FL_ERR_ALIGN;
    SelectArgs a;
    // err_flag for a uniform-width column too, the only consumer that takes one: this form raises FL_DEVERR_BOUNDS (a run outside `out`)
    const WaveShape sh = block_consumer_args<T>(a, col, packed, ref_stride, n_blocks, err_flag);
    a.mask = mask;
    a.out_offsets = out_offsets;
    a.out = reinterpret_cast<char*>(out);
    a.out_len = out_len;
    a.sel_refs = refs;
    return hip_status(select_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_aggregate (fl_aggregate.hpp: a block that fails the kernel's checks leaves the identity in its slot).  Launched with the shape of
// unfor_pack_widths, as unfor_select is.  `mask` may be NULL: every row is kept and no mask is read.
template <typename T>
int run_unfor_aggregate(const Column& col, const T* packed, const T* refs, size_t ref_stride, const uint32_t* mask, size_t n_blocks,
                        void* block_aggs, uint32_t* err_flag, void* stream)
{
    if (!col.mixed && over_width<T>(col.width)) return FL_ERR_WIDTH;
    if (n_blocks == 0) return FL_OK;
    if (!block_consumer_column(col, packed, refs) || !block_aggs) return FL_ERR_NULL;
    if (misaligned(packed) || misaligned(mask) || misaligned(block_aggs)) return FL_ERR_ALIGN;
    AggregateArgs a;
    const WaveShape sh = block_consumer_args<T>(a, col, packed, ref_stride, n_blocks, col.mixed ? err_flag : nullptr);
    a.mask = mask;
    a.aggs = static_cast<char*>(block_aggs);
    a.agg_refs = refs;
    return hip_status(aggregate_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_aggregate_columns (fl_aggregate_columns.hpp): two columns of T of the same form, both uniform or both mixed, met element by
// element under `expr` and aggregated per block as run_unfor_aggregate does (a block that fails either column's checks leaves the
// identity in its slot).  The same launch shape; the checks in the order of run_unfor_aggregate, `expr` where a `combine` is judged.
template <typename T>
int run_unfor_aggregate_columns(int expr, const Column& cola, const T* a_packed, const T* a_refs, size_t a_ref_stride, const Column& colb,
                                const T* b_packed, const T* b_refs, size_t b_ref_stride, const uint32_t* mask, size_t n_blocks,
                                void* block_aggs, uint32_t* err_flag, void* stream)
{
    if ((!cola.mixed && over_width<T>(cola.width)) || (!colb.mixed && over_width<T>(colb.width))) return FL_ERR_WIDTH;
    if (!expr_valid(expr)) return FL_ERR_INDEX;
    if (n_blocks == 0) return FL_OK;
    if (!block_consumer_column(cola, a_packed, a_refs) || !block_consumer_column(colb, b_packed, b_refs) || !block_aggs) return FL_ERR_NULL;
    if (misaligned(a_packed) || misaligned(b_packed) || misaligned(mask) || misaligned(block_aggs)) return FL_ERR_ALIGN;
    AggregateColumnsArgs a;
    uint32_t* ef = cola.mixed ? err_flag : nullptr;
    const WaveShape sh = block_consumer_args<T>(a, cola, a_packed, a_ref_stride, n_blocks, ef);
    block_consumer_args<T>(a.b, colb, b_packed, b_ref_stride, n_blocks, ef);
    a.mask = mask;
    a.aggs = static_cast<char*>(block_aggs);
    a.agg_refs = a_refs;
    a.b_refs = b_refs;
    a.expr = (unsigned)expr;
    return hip_status(aggregate_columns_launcher<T>()(a, sh.waves, static_cast<hipStream_t>(stream)));
}

// unfor_aggregate_by (fl_aggregate_by.hpp): a value column of T and a u8 key column of the same form, both uniform or both mixed; a
// block that fails either column's checks contributes nothing.  `result` (256 slots) is written by EVERY call -- the init launch also
// answers an empty column -- so it is required and checked before the empty-column return.  The persistent grid takes the policy's
// waves as its residency and the policy's blocks per wavefront as the least length of a wavefront's run (0: the column divided evenly).
template <typename T>
int run_unfor_aggregate_by(const Column& col, const T* packed, const T* refs, size_t ref_stride, const Column& kcol, const uint8_t* keys,
                           const uint8_t* key_refs, size_t key_ref_stride, const uint32_t* mask, size_t n_blocks, void* result,
                           uint32_t* err_flag, void* stream)
{
    if ((!col.mixed && over_width<T>(col.width)) || (!kcol.mixed && over_width<uint8_t>(kcol.width))) return FL_ERR_WIDTH;
    if (!result) return FL_ERR_NULL;
    if (n_blocks && (!block_consumer_column(col, packed, refs) || !block_consumer_column(kcol, keys, key_refs))) return FL_ERR_NULL;
    if ((n_blocks && (misaligned(packed) || misaligned(keys) || misaligned(mask))) || misaligned(result)) return FL_ERR_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipError_t e = launch_aggregate_by_init(static_cast<BlockAggregate*>(result), s); e != hipSuccess || n_blocks == 0) return hip_status(e);
    const WaveShape sh = with_policy({0, 0u, 0u});
    AggregateByArgs a;
    widths_args<T>(a.val, col, packed, nullptr, nullptr, ref_stride, col.mixed ? err_flag : nullptr, n_blocks, sh);
    widths_args<uint8_t>(a.key, kcol, keys, nullptr, nullptr, key_ref_stride, col.mixed ? err_flag : nullptr, n_blocks, sh);
    a.val_refs = refs;
    a.key_refs = key_refs;
    a.mask = mask;
    a.result = static_cast<BlockAggregate*>(result);
    a.run = 0;
    return hip_status(aggregate_by_launcher<T>()(a, sh.waves, s));
}

// unfor_aggregate_by_columns (fl_aggregate_by_columns.hpp): two value columns of T met under `expr` and a u8 key column, all three of
// the same form, uniform or mixed; a block that fails any column's checks contributes nothing.  The checks of run_unfor_aggregate_by
// in its order, `expr` where run_unfor_aggregate_columns judges it; `result` and the persistent grid as run_unfor_aggregate_by has them.
template <typename T>
int run_unfor_aggregate_by_columns(int expr, const Column& cola, const T* a_packed, const T* a_refs, size_t a_ref_stride, const Column& colb,
                                   const T* b_packed, const T* b_refs, size_t b_ref_stride, const Column& kcol, const uint8_t* keys,
                                   const uint8_t* key_refs, size_t key_ref_stride, const uint32_t* mask, size_t n_blocks, void* result,
                                   uint32_t* err_flag, void* stream)
{
    if ((!cola.mixed && over_width<T>(cola.width)) || (!colb.mixed && over_width<T>(colb.width)) || (!kcol.mixed && over_width<uint8_t>(kcol.width)))
        return FL_ERR_WIDTH;
    if (!expr_valid(expr)) return FL_ERR_INDEX;
    if (!result) return FL_ERR_NULL;
    if (n_blocks && (!block_consumer_column(cola, a_packed, a_refs) || !block_consumer_column(colb, b_packed, b_refs) ||
                     !block_consumer_column(kcol, keys, key_refs)))
        return FL_ERR_NULL;
    if ((n_blocks && (misaligned(a_packed) || misaligned(b_packed) || misaligned(keys) || misaligned(mask))) || misaligned(result)) return FL_ERR_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipError_t e = launch_aggregate_by_init(static_cast<BlockAggregate*>(result), s); e != hipSuccess || n_blocks == 0) return hip_status(e);
    const WaveShape sh = with_policy({0, 0u, 0u});
    AggregateByColumnsArgs a;
    uint32_t* ef = cola.mixed ? err_flag : nullptr;
    widths_args<T>(a.a, cola, a_packed, nullptr, nullptr, a_ref_stride, ef, n_blocks, sh);
    widths_args<T>(a.b, colb, b_packed, nullptr, nullptr, b_ref_stride, ef, n_blocks, sh);
    widths_args<uint8_t>(a.key, kcol, keys, nullptr, nullptr, key_ref_stride, ef, n_blocks, sh);
    a.a_refs = a_refs;
    a.b_refs = b_refs;
    a.key_refs = key_refs;
    a.mask = mask;
    a.result = static_cast<BlockAggregate*>(result);
    a.run = 0;
    a.expr = (unsigned)expr;
    return hip_status(aggregate_by_columns_launcher<T>()(a, sh.waves, s));
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
    int fl_##S##_unfor_compare(unsigned w, const T* in, const T* r, size_t rs, int op, T k, size_t n, uint32_t* mask, void* s) \
    { FL_DEVICE_TIER(s, in, r, mask); return run_unfor_compare<T>({false, w}, in, r, rs, op, k, n, mask, nullptr, s); } \
    int fl_##S##_unfor_compare_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, int op, T k, \
                                      size_t n, uint32_t* mask, uint32_t* ef, void* s)                   \
    { FL_DEVICE_TIER(s, w, o, pk, r, mask, ef); return run_unfor_compare<T>({true, 0, w, o, pb}, pk, r, rs, op, k, n, mask, ef, s); }     \
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

#define FL_DEFINE_SELECT(T, S)                                                                            \
    int fl_##S##_unfor_select(unsigned w, const T* in, const T* r, size_t rs, const uint32_t* mask, const uint64_t* oo, T* out, size_t ol, \
                              size_t n, uint32_t* ef, void* s)                                            \
    { FL_DEVICE_TIER(s, in, r, mask, oo, out, ef); return run_unfor_select<T>({false, w}, in, r, rs, mask, oo, out, ol, n, ef, s); } \
    int fl_##S##_unfor_select_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, const uint32_t* mask, \
                                     const uint64_t* oo, T* out, size_t ol, size_t n, uint32_t* ef, void* s) \
    { FL_DEVICE_TIER(s, w, o, pk, r, mask, oo, out, ef); return run_unfor_select<T>({true, 0, w, o, pb}, pk, r, rs, mask, oo, out, ol, n, ef, s); }

FL_DEFINE_SELECT(uint8_t, u8)
FL_DEFINE_SELECT(uint16_t, u16)
FL_DEFINE_SELECT(uint32_t, u32)
FL_DEFINE_SELECT(uint64_t, u64)

#define FL_DEFINE_AGGREGATE(T, S)                                                                         \
    int fl_##S##_unfor_aggregate(unsigned w, const T* in, const T* r, size_t rs, const uint32_t* mask, size_t n, void* aggs, uint32_t* ef, \
                                 void* s)                                                                 \
    { FL_DEVICE_TIER(s, in, r, mask, aggs, ef); return run_unfor_aggregate<T>({false, w}, in, r, rs, mask, n, aggs, ef, s); } \
    int fl_##S##_unfor_aggregate_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, const uint32_t* mask, \
                                        size_t n, void* aggs, uint32_t* ef, void* s)                      \
    { FL_DEVICE_TIER(s, w, o, pk, r, mask, aggs, ef); return run_unfor_aggregate<T>({true, 0, w, o, pb}, pk, r, rs, mask, n, aggs, ef, s); }

FL_DEFINE_AGGREGATE(uint8_t, u8)
FL_DEFINE_AGGREGATE(uint16_t, u16)
FL_DEFINE_AGGREGATE(uint32_t, u32)
FL_DEFINE_AGGREGATE(uint64_t, u64)

#define FL_DEFINE_AGGREGATE_BY(T, S)                                                                      \
    int fl_##S##_unfor_aggregate_by(unsigned w, const T* in, const T* r, size_t rs, unsigned kw, const uint8_t* k, const uint8_t* kr, size_t krs, \
                                    const uint32_t* mask, size_t n, void* res, uint32_t* ef, void* s)     \
    {                                                                                                     \
        FL_DEVICE_TIER(s, in, r, k, kr, mask, res, ef);                                                   \
        return run_unfor_aggregate_by<T>({false, w}, in, r, rs, {false, kw}, k, kr, krs, mask, n, res, ef, s); \
    }                                                                                                     \
    int fl_##S##_unfor_aggregate_by_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, const uint8_t* kw, \
                                           const uint64_t* ko, const uint8_t* k, size_t kb, const uint8_t* kr, size_t krs, const uint32_t* mask, \
                                           size_t n, void* res, uint32_t* ef, void* s)                    \
    {                                                                                                     \
        FL_DEVICE_TIER(s, w, o, pk, r, kw, ko, k, kr, mask, res, ef);                                     \
        return run_unfor_aggregate_by<T>({true, 0, w, o, pb}, pk, r, rs, {true, 0, kw, ko, kb}, k, kr, krs, mask, n, res, ef, s); \
    }

FL_DEFINE_AGGREGATE_BY(uint8_t, u8)
FL_DEFINE_AGGREGATE_BY(uint16_t, u16)
FL_DEFINE_AGGREGATE_BY(uint32_t, u32)
FL_DEFINE_AGGREGATE_BY(uint64_t, u64)

#define FL_DEFINE_AGGREGATE_BY_COLUMNS(T, S)                                                              \
    int fl_##S##_unfor_aggregate_by_columns(int ex, unsigned wa, const T* a, const T* ar, size_t ars, unsigned wb, const T* b, const T* br, \
                                            size_t brs, unsigned kw, const uint8_t* k, const uint8_t* kr, size_t krs, const uint32_t* mask, \
                                            size_t n, void* res, uint32_t* ef, void* s)                   \
    {                                                                                                     \
        FL_DEVICE_TIER(s, a, ar, b, br, k, kr, mask, res, ef);                                            \
        return run_unfor_aggregate_by_columns<T>(ex, {false, wa}, a, ar, ars, {false, wb}, b, br, brs, {false, kw}, k, kr, krs, mask, n, res, ef, s); \
    }                                                                                                     \
    int fl_##S##_unfor_aggregate_by_columns_widths(int ex, const uint8_t* aw, const uint64_t* ao, const T* a, size_t ab, const T* ar, size_t ars, \
                                                   const uint8_t* bw, const uint64_t* bo, const T* b, size_t bb, const T* br, size_t brs, \
                                                   const uint8_t* kw, const uint64_t* ko, const uint8_t* k, size_t kb, const uint8_t* kr, \
                                                   size_t krs, const uint32_t* mask, size_t n, void* res, uint32_t* ef, void* s) \
    {                                                                                                     \
        FL_DEVICE_TIER(s, aw, ao, a, ar, bw, bo, b, br, kw, ko, k, kr, mask, res, ef);                    \
        return run_unfor_aggregate_by_columns<T>(ex, {true, 0, aw, ao, ab}, a, ar, ars, {true, 0, bw, bo, bb}, b, br, brs, {true, 0, kw, ko, kb}, k, \
                                                 kr, krs, mask, n, res, ef, s);                           \
    }

FL_DEFINE_AGGREGATE_BY_COLUMNS(uint8_t, u8)
FL_DEFINE_AGGREGATE_BY_COLUMNS(uint16_t, u16)
FL_DEFINE_AGGREGATE_BY_COLUMNS(uint32_t, u32)
FL_DEFINE_AGGREGATE_BY_COLUMNS(uint64_t, u64)

#define FL_DEFINE_SET_BUILD(T, S)                                                                         \
    int fl_##S##_unfor_set_build(unsigned w, const T* in, const T* r, size_t rs, const uint32_t* mask, size_t n, T lo, uint64_t sb, \
                                 uint32_t* sw, uint64_t* st, void* s)                                     \
    { FL_DEVICE_TIER(s, in, r, mask, sw, st); return run_unfor_set_build<T>({false, w}, in, r, rs, mask, n, lo, sb, sw, st, nullptr, s); } \
    int fl_##S##_unfor_set_build_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, const uint32_t* mask, \
                                        size_t n, T lo, uint64_t sb, uint32_t* sw, uint64_t* st, uint32_t* ef, void* s) \
    { FL_DEVICE_TIER(s, w, o, pk, r, mask, sw, st, ef); return run_unfor_set_build<T>({true, 0, w, o, pb}, pk, r, rs, mask, n, lo, sb, sw, st, ef, s); }

FL_DEFINE_SET_BUILD(uint8_t, u8)
FL_DEFINE_SET_BUILD(uint16_t, u16)
FL_DEFINE_SET_BUILD(uint32_t, u32)
FL_DEFINE_SET_BUILD(uint64_t, u64)

#define FL_DEFINE_AGGREGATE_BY_WINDOW(T, S)                                                               \
    int fl_##S##_unfor_aggregate_by_window(unsigned w, const T* in, const T* r, size_t rs, unsigned kw, const T* k, const T* kr, size_t krs, \
                                           const uint32_t* mask, size_t n, T lo, uint64_t ng, uint64_t* cn, uint64_t* sm, uint64_t* mn, \
                                           uint64_t* mx, uint64_t* st, void* s)                           \
    {                                                                                                     \
        FL_DEVICE_TIER(s, in, r, k, kr, mask, cn, sm, mn, mx, st);                                        \
        return run_unfor_aggregate_by_window<T>({false, w}, in, r, rs, {false, kw}, k, kr, krs, mask, n, lo, ng, {cn, sm, mn, mx, st}, nullptr, s); \
    }                                                                                                     \
    int fl_##S##_unfor_aggregate_by_window_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, \
                                                  const uint8_t* kw, const uint64_t* ko, const T* k, size_t kb, const T* kr, size_t krs, \
                                                  const uint32_t* mask, size_t n, T lo, uint64_t ng, uint64_t* cn, uint64_t* sm, uint64_t* mn, \
                                                  uint64_t* mx, uint64_t* st, uint32_t* ef, void* s)      \
    {                                                                                                     \
        FL_DEVICE_TIER(s, w, o, pk, r, kw, ko, k, kr, mask, cn, sm, mn, mx, st, ef);                      \
        return run_unfor_aggregate_by_window<T>({true, 0, w, o, pb}, pk, r, rs, {true, 0, kw, ko, kb}, k, kr, krs, mask, n, lo, ng, \
                                                {cn, sm, mn, mx, st}, ef, s);                             \
    }

FL_DEFINE_AGGREGATE_BY_WINDOW(uint8_t, u8)
FL_DEFINE_AGGREGATE_BY_WINDOW(uint16_t, u16)
FL_DEFINE_AGGREGATE_BY_WINDOW(uint32_t, u32)
FL_DEFINE_AGGREGATE_BY_WINDOW(uint64_t, u64)

#define FL_DEFINE_LOOKUP_FORMS(T, S, U, NAME)                                                              \
    int fl_##S##_##NAME(unsigned w, const T* in, const T* r, size_t rs, const uint32_t* mask, size_t n, T lo, uint64_t ns, const U* tb, \
                        const uint32_t* pr, U ms, U* out, uint32_t* hm, uint64_t* st, void* s)            \
    {                                                                                                     \
        FL_DEVICE_TIER(s, in, r, mask, tb, pr, out, hm, st);                                              \
        return run_unfor_lookup<T>({false, w}, in, r, rs, mask, n, lo, ns, (unsigned)sizeof(U), {tb, pr, ms, out, hm, st}, nullptr, s); \
    }                                                                                                     \
    int fl_##S##_##NAME##_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, const uint32_t* mask, \
                                 size_t n, T lo, uint64_t ns, const U* tb, const uint32_t* pr, U ms, U* out, uint32_t* hm, uint64_t* st, \
                                 uint32_t* ef, void* s)                                                   \
    {                                                                                                     \
        FL_DEVICE_TIER(s, w, o, pk, r, mask, tb, pr, out, hm, st, ef);                                    \
        return run_unfor_lookup<T>({true, 0, w, o, pb}, pk, r, rs, mask, n, lo, ns, (unsigned)sizeof(U), {tb, pr, ms, out, hm, st}, ef, s); \
    }
#define FL_DEFINE_LOOKUP(T, S) FL_DEFINE_LOOKUP_FORMS(T, S, T, unfor_lookup)
#define FL_DEFINE_LOOKUP_U8(T, S) FL_DEFINE_LOOKUP_FORMS(T, S, uint8_t, unfor_lookup_u8)

FL_DEFINE_LOOKUP(uint8_t, u8)
FL_DEFINE_LOOKUP(uint16_t, u16)
FL_DEFINE_LOOKUP(uint32_t, u32)
FL_DEFINE_LOOKUP(uint64_t, u64)
FL_DEFINE_LOOKUP_U8(uint8_t, u8)
FL_DEFINE_LOOKUP_U8(uint16_t, u16)
FL_DEFINE_LOOKUP_U8(uint32_t, u32)
FL_DEFINE_LOOKUP_U8(uint64_t, u64)

#define FL_DEFINE_AGGREGATE_BY_LOOKUP(T, S)                                                               \
    int fl_##S##_unfor_aggregate_by_lookup(unsigned w, const T* in, const T* r, size_t rs, unsigned kw, const T* k, const T* kr, size_t krs, \
                                           const uint32_t* mask, size_t n, T lo, uint64_t ns, const uint8_t* tb, const uint32_t* pr, void* res, \
                                           uint64_t* st, uint32_t* ef, void* s)                           \
    {                                                                                                     \
        FL_DEVICE_TIER(s, in, r, k, kr, mask, tb, pr, res, st, ef);                                       \
        return run_unfor_aggregate_by_lookup<T>({false, w}, in, r, rs, {false, kw}, k, kr, krs, mask, n, lo, ns, {tb, pr, res, st}, ef, s); \
    }                                                                                                     \
    int fl_##S##_unfor_aggregate_by_lookup_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, \
                                                  const uint8_t* kw, const uint64_t* ko, const T* k, size_t kb, const T* kr, size_t krs, \
                                                  const uint32_t* mask, size_t n, T lo, uint64_t ns, const uint8_t* tb, const uint32_t* pr, \
                                                  void* res, uint64_t* st, uint32_t* ef, void* s)         \
    {                                                                                                     \
        FL_DEVICE_TIER(s, w, o, pk, r, kw, ko, k, kr, mask, tb, pr, res, st, ef);                         \
        return run_unfor_aggregate_by_lookup<T>({true, 0, w, o, pb}, pk, r, rs, {true, 0, kw, ko, kb}, k, kr, krs, mask, n, lo, ns, \
                                                {tb, pr, res, st}, ef, s);                                \
    }

FL_DEFINE_AGGREGATE_BY_LOOKUP(uint8_t, u8)
FL_DEFINE_AGGREGATE_BY_LOOKUP(uint16_t, u16)
FL_DEFINE_AGGREGATE_BY_LOOKUP(uint32_t, u32)
FL_DEFINE_AGGREGATE_BY_LOOKUP(uint64_t, u64)

#define FL_DEFINE_FOR_COMPARE_RANGE(T, S)                                                               \
    int fl_##S##_unfor_compare_range(unsigned w, const T* in, const T* r, size_t rs, T lo, T hi, int cb, const uint32_t* mi, size_t n, \
                                     uint32_t* mask, void* s)                                             \
    { FL_DEVICE_TIER(s, in, r, mi, mask); return run_unfor_compare_range<T>({false, w}, in, r, rs, lo, hi, cb, mi, n, mask, nullptr, s); } \
    int fl_##S##_unfor_compare_range_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, T lo, T hi, \
                                            int cb, const uint32_t* mi, size_t n, uint32_t* mask, uint32_t* ef, void* s) \
    { FL_DEVICE_TIER(s, w, o, pk, r, mi, mask, ef); return run_unfor_compare_range<T>({true, 0, w, o, pb}, pk, r, rs, lo, hi, cb, mi, n, mask, ef, s); }

FL_DEFINE_FOR_COMPARE_RANGE(uint8_t, u8)
FL_DEFINE_FOR_COMPARE_RANGE(uint16_t, u16)
FL_DEFINE_FOR_COMPARE_RANGE(uint32_t, u32)
FL_DEFINE_FOR_COMPARE_RANGE(uint64_t, u64)

#define FL_DEFINE_DELTA_COMPARE_RANGE(T, S)                                                             \
    int fl_##S##_undelta_compare_range(unsigned w, const T* in, const T* b, T lo, T hi, int cb, const uint32_t* mi, size_t n, uint32_t* mask, \
                                       void* s)                                                           \
    { FL_DEVICE_TIER(s, in, b, mi, mask); return run_undelta_compare_range<T>({false, w}, in, b, lo, hi, cb, mi, n, mask, nullptr, s); } \
    int fl_##S##_undelta_compare_range_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* b, T lo, T hi, int cb, \
                                              const uint32_t* mi, size_t n, uint32_t* mask, uint32_t* ef, void* s) \
    { FL_DEVICE_TIER(s, w, o, pk, b, mi, mask, ef); return run_undelta_compare_range<T>({true, 0, w, o, pb}, pk, b, lo, hi, cb, mi, n, mask, ef, s); }

FL_DEFINE_DELTA_COMPARE_RANGE(uint8_t, u8)
FL_DEFINE_DELTA_COMPARE_RANGE(uint16_t, u16)
FL_DEFINE_DELTA_COMPARE_RANGE(uint32_t, u32)
FL_DEFINE_DELTA_COMPARE_RANGE(uint64_t, u64)

#define FL_DEFINE_FOR_COMPARE_IN(T, S)                                                                    \
    int fl_##S##_unfor_compare_in(unsigned w, const T* in, const T* r, size_t rs, T lo, uint64_t sb, const uint32_t* sw, int ng, int cb, \
                                  const uint32_t* mi, size_t n, uint32_t* mask, void* s)                  \
    { FL_DEVICE_TIER(s, in, r, sw, mi, mask); return run_unfor_compare_in<T>({false, w}, in, r, rs, lo, sb, sw, ng, cb, mi, n, mask, nullptr, s); } \
    int fl_##S##_unfor_compare_in_widths(const uint8_t* w, const uint64_t* o, const T* pk, size_t pb, const T* r, size_t rs, T lo, uint64_t sb, \
                                         const uint32_t* sw, int ng, int cb, const uint32_t* mi, size_t n, uint32_t* mask, uint32_t* ef, void* s) \
    { FL_DEVICE_TIER(s, w, o, pk, r, sw, mi, mask, ef); return run_unfor_compare_in<T>({true, 0, w, o, pb}, pk, r, rs, lo, sb, sw, ng, cb, mi, n, mask, ef, s); }

FL_DEFINE_FOR_COMPARE_IN(uint8_t, u8)
FL_DEFINE_FOR_COMPARE_IN(uint16_t, u16)
FL_DEFINE_FOR_COMPARE_IN(uint32_t, u32)
FL_DEFINE_FOR_COMPARE_IN(uint64_t, u64)

#define FL_DEFINE_FOR_COMPARE_COLUMNS(T, S)                                                               \
    int fl_##S##_unfor_compare_columns(unsigned wa, const T* a, const T* ar, size_t ars, unsigned wb, const T* b, const T* br, size_t brs, \
                                       int op, int sg, int cb, const uint32_t* mi, size_t n, uint32_t* mask, void* s) \
    {                                                                                                     \
        FL_DEVICE_TIER(s, a, ar, b, br, mi, mask);                                                        \
        return run_unfor_compare_columns<T>({false, wa}, a, ar, ars, {false, wb}, b, br, brs, op, sg, cb, mi, n, mask, nullptr, s); \
    }                                                                                                     \
    int fl_##S##_unfor_compare_columns_widths(const uint8_t* aw, const uint64_t* ao, const T* a, size_t ab, const T* ar, size_t ars, \
                                              const uint8_t* bw, const uint64_t* bo, const T* b, size_t bb, const T* br, size_t brs, \
                                              int op, int sg, int cb, const uint32_t* mi, size_t n, uint32_t* mask, uint32_t* ef, void* s) \
    {                                                                                                     \
        FL_DEVICE_TIER(s, aw, ao, a, ar, bw, bo, b, br, mi, mask, ef);                                    \
        return run_unfor_compare_columns<T>({true, 0, aw, ao, ab}, a, ar, ars, {true, 0, bw, bo, bb}, b, br, brs, op, sg, cb, mi, n, mask, ef, s); \
    }

FL_DEFINE_FOR_COMPARE_COLUMNS(uint8_t, u8)
FL_DEFINE_FOR_COMPARE_COLUMNS(uint16_t, u16)
FL_DEFINE_FOR_COMPARE_COLUMNS(uint32_t, u32)
FL_DEFINE_FOR_COMPARE_COLUMNS(uint64_t, u64)

#define FL_DEFINE_AGGREGATE_COLUMNS(T, S)                                                                 \
    int fl_##S##_unfor_aggregate_columns(int ex, unsigned wa, const T* a, const T* ar, size_t ars, unsigned wb, const T* b, const T* br, \
                                         size_t brs, const uint32_t* mask, size_t n, void* aggs, uint32_t* ef, void* s) \
    {                                                                                                     \
        FL_DEVICE_TIER(s, a, ar, b, br, mask, aggs, ef);                                                  \
        return run_unfor_aggregate_columns<T>(ex, {false, wa}, a, ar, ars, {false, wb}, b, br, brs, mask, n, aggs, ef, s); \
    }                                                                                                     \
    int fl_##S##_unfor_aggregate_columns_widths(int ex, const uint8_t* aw, const uint64_t* ao, const T* a, size_t ab, const T* ar, size_t ars, \
                                                const uint8_t* bw, const uint64_t* bo, const T* b, size_t bb, const T* br, size_t brs, \
                                                const uint32_t* mask, size_t n, void* aggs, uint32_t* ef, void* s) \
    {                                                                                                     \
        FL_DEVICE_TIER(s, aw, ao, a, ar, bw, bo, b, br, mask, aggs, ef);                                  \
        return run_unfor_aggregate_columns<T>(ex, {true, 0, aw, ao, ab}, a, ar, ars, {true, 0, bw, bo, bb}, b, br, brs, mask, n, aggs, ef, s); \
    }

FL_DEFINE_AGGREGATE_COLUMNS(uint8_t, u8)
FL_DEFINE_AGGREGATE_COLUMNS(uint16_t, u16)
FL_DEFINE_AGGREGATE_COLUMNS(uint32_t, u32)
FL_DEFINE_AGGREGATE_COLUMNS(uint64_t, u64)

FL_DEFINE_TYPE(uint8_t, u8)
FL_DEFINE_TYPE(uint16_t, u16)
FL_DEFINE_TYPE(uint32_t, u32)
FL_DEFINE_TYPE(uint64_t, u64)


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
