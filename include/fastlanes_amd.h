/*
 * fastlanes_amd.h -- C ABI of the MI355X-native FastLanes codec (libfastlanes_amd.so).
 *
 * The drop-in boundary for spiraldb/fastlanes' BitPacking / FoR / Delta /
 * Transpose trait methods (reference: /root/reference/src).  The Rust traits
 * are static methods monomorphised per element type and const width W; an FFI
 * cannot carry const generics, so every entry point takes the runtime `width`
 * exactly like the reference's own `unchecked_*` methods do
 * (bitpacking.rs:30,44,58) and dispatches to a per-(T,W) gfx950 kernel.
 *
 * Naming:  fl_<ty>_<method>[_host],  <ty> in {u8,u16,u32,u64},  <method> the
 * reference's method name.  Each function cites the reference interface it
 * replaces.
 *
 * Two tiers, same kernels:
 *   DEVICE tier  fl_<ty>_<method>(..., n_blocks, stream)
 *       All data pointers are DEVICE pointers (HBM).  The op is applied to
 *       n_blocks contiguous 1024-value blocks: block b reads
 *       in + b*in_block_elems and writes out + b*out_block_elems, where an
 *       unpacked block is 1024 elements and a packed block is 1024*W/T elements
 *       (= 128*W bytes; bitpacking.rs:77).  This is the reference's caller loop
 *       (benches/bitpacking.rs:80-97) moved on-device.  Asynchronous on `stream`
 *       (a hipStream_t, passed as void*; NULL = default stream); never
 *       synchronises, never allocates, retains no pointer.
 *   HOST tier    fl_<ty>_<method>_host(..., n_blocks)
 *       Same semantics with HOST pointers (the trait methods' `&[T]` slices,
 *       e.g. bitpacking.rs:19,33): runs the same kernels on the calling
 *       thread's current device and synchronises before returning.  n_blocks = 1
 *       is the exact shape of one trait-method call.  Small calls are zero-copy
 *       (the kernel reads/writes a pinned host buffer over PCIe; the calling
 *       thread polls a completion word in pinned memory for the ~10 us the call
 *       takes, whatever the device's scheduling flags say); large calls
 *       stage through a cached device buffer; after a thread's first call
 *       nothing is allocated (fl_host_release).  There is no CPU code path:
 *       without a GPU these return FL_ERR_HIP.
 *
 * Preconditions.  Device pointers 16-byte aligned (every block is a multiple
 * of 128 bytes, so block starts stay aligned; 128-byte alignment of the
 * column base is recommended for full-line accesses).  in/out must not
 * overlap.  width <= T.  Outputs are fully overwritten (pack with width 0
 * writes nothing, macros.rs:52-53; unpack with width 0 writes 1024 zeros per
 * block, macros.rs:118-125).
 *
 * Errors.  The reference has no Result type: `unchecked_*` panics via
 * unreachable!() on width > T (bitpacking.rs:93,126,197) and unpack_single
 * asserts index < 1024 (bitpacking.rs:152).  Here every function returns an
 * fl_status; a binding maps nonzero to panic! to match.
 * Nothing throws or aborts across the ABI.  Every launch first CLEARS the calling
 * thread's pending HIP error (hipGetLastError) so that FL_ERR_HIP always means this
 * call's launch failed, never an earlier benign failure of the application's own
 * HIP calls: an application that relies on hipGetLastError across a call into this
 * library must read it before the call.
 *
 * Threading and device selection.  Re-entrant and thread-safe.  The library's own
 * state: per host thread, the host tier's context (stream and staging buffers,
 * fl_host_release); per device, the grid sizes of the persistent kernels; per
 * process, the kernel-policy and tile-map overrides of fastlanes_amd_internal.h,
 * and for fl_column_pair_alloc the registry of live FL_LAYOUT_INTERLEAVED pairs,
 * the address ranges such pairs have used and a chunk cache (empty unless a tool
 * enables it).  No entry point changes the calling thread's current device
 * (fl_column_pair_free switches to the pair's device for a moment and switches
 * back).  The device is selected the way HIP selects it: kernels run on the
 * device that is CURRENT for the calling thread, so `stream` (when not NULL)
 * must be a stream of that device and every device pointer must be memory that
 * device can use (its own HBM, managed memory, or pinned host memory).  One host
 * thread per device, each after its own hipSetDevice, is the intended multi-GPU
 * shape (examples/multi_gpu_decode.c).
 * A mismatch -- device 0 current, buffers or stream of device 1 -- is undefined
 * behaviour by default, exactly as for a raw kernel launch; with the environment
 * variable FL_CHECK_DEVICE=1 (read once, at the first device-tier call) every
 * device-tier entry point verifies it with hipPointerGetAttributes /
 * hipStreamGetDevice before launching and returns FL_ERR_DEVICE instead: a debug
 * aid that costs a few microseconds per call.
 */
#ifndef FASTLANES_AMD_H
#define FASTLANES_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum fl_status {
    FL_OK = 0,
    FL_ERR_WIDTH = 1,   /* width > T              (bitpacking.rs:93 unreachable!) */
    FL_ERR_INDEX = 2,   /* index >= 1024*n_blocks (bitpacking.rs:152 assert!)      */
    FL_ERR_NULL = 3,    /* required pointer is NULL                                */
    FL_ERR_ALIGN = 4,   /* device pointer not 16-byte aligned (fl_fill_random: 8)  */
    FL_ERR_HIP = 5,     /* HIP runtime error; see fl_last_hip_error()              */
    FL_ERR_BOUNDS = 6,  /* a block's bytes lie outside the packed column           */
    FL_ERR_DEVICE = 7   /* FL_CHECK_DEVICE=1 only: a device-tier pointer is not memory the
                           calling thread's current device can use, or `stream` belongs to
                           another device (see "Threading")                        */
} fl_status;

/* Device-side error bits.  The device tier never synchronises, so what the reference reports by panicking in the middle
 * of a caller loop (bitpacking.rs:93,126,152,197 and the debug_asserts on lengths :78-80,111-113,185-186) is reported
 * through *err_flag (a device uint32 the caller zeroes; may be NULL): the offending block / index is SKIPPED (a lookup
 * writes 0) and its bit is ORed in. */
enum {
    FL_DEVERR_WIDTH = 1,   /* widths[b] > T                                              -> FL_ERR_WIDTH  */
    FL_DEVERR_INDEX = 2,   /* lookup index >= 1024*n_blocks                              -> FL_ERR_INDEX  */
    FL_DEVERR_ALIGN = 4,   /* offsets[b] not a multiple of 16 (lookups: of sizeof(T))    -> FL_ERR_ALIGN  */
    FL_DEVERR_BOUNDS = 8   /* offsets[b] + 128*widths[b] > packed_bytes                  -> FL_ERR_BOUNDS */
};

/* predicates of fl_<ty>_unpack_compare (unsigned comparison with a constant) */
typedef enum fl_cmp { FL_CMP_EQ = 0, FL_CMP_NE = 1, FL_CMP_LT = 2, FL_CMP_LE = 3, FL_CMP_GT = 4, FL_CMP_GE = 5 } fl_cmp;

/* Library / build identification and diagnostics. */
const char *fl_version(void);
const char *fl_status_string(int status);
/* hipError_t of the most recent FL_ERR_HIP on the calling thread (0 if none). */
int fl_last_hip_error(void);
/* Elements in one packed block: 1024*width/T (bitpacking.rs:77); 0 if width > T. */
size_t fl_packed_len(unsigned type_bits, unsigned width);
/* The host tier keeps one cached context per calling thread (a private stream, a pinned staging
 * buffer, a device scratch buffer; see "HOST tier" above) so that its calls allocate nothing after
 * the first one, like the allocation-free reference (lib.rs:3).  It is freed at thread exit; this
 * frees the calling thread's context early (long-lived worker threads should call it before they exit: at process
 * teardown the destructor frees nothing if the HIP runtime no longer answers). */
void fl_host_release(void);
/* (The kernel-selection override used by the parity tests and the A/B tools is NOT part of this interface:
 * include/fastlanes_amd_internal.h.) */

/* Test / benchmark data generated in HBM (not a reference function; SURVEY.md 8(d) asks for a counter-based generator
 * so that a host can regenerate any part of a device-resident column without a PCIe transfer): 64-bit word i of dst =
 * output number i+1 of splitmix64 seeded with seed * 0x9E3779B97F4A7C15.  dst 8-byte aligned, n_bytes a multiple of 8
 * (FL_ERR_ALIGN otherwise).  Asynchronous on `stream`. */
int fl_fill_random(void *dst, size_t n_bytes, uint64_t seed, void *stream);

/*
 * OPTIONAL allocation helper -- never needed to use the codec: every entry point takes any 16-byte aligned device pointers and
 * allocates nothing.  It exists because WHERE a column's buffers live in HBM moves every streaming kernel by a few per cent on
 * MI355X (the same kernel, the same bytes, another allocation: 0.78-0.86 of the peak), nothing in an address
 * tells which, and a caller that allocates a (packed, unpacked) pair it is going to stream through many times can MEASURE it once:
 *   FL_LAYOUT_SEPARATE     one hipMalloc per buffer, wherever the driver puts them
 *   FL_LAYOUT_ZONED        one hipMalloc; `in` (then `aux`) at its start, `out` centred on the first 64-GiB multiple that leaves room
 *                          for them.  COSTS THE UNUSED BYTES IN BETWEEN: the allocation is about 64 GiB + out_bytes / 2 whatever the
 *                          pair's size (a multiple of 64 GiB more for inputs beyond ~60 GiB) -- a few such pairs exhaust a device.
 *   FL_LAYOUT_INTERLEAVED  CONSTRUCTED (round 6; DESIGN.md section 4, profiles/r06_vmm_placement.txt): the pair is built from 1-GiB
 *                          physical chunks (hipMemCreate) mapped into ONE address range (hipMemAddressReserve / hipMemMap).  The device
 *                          memory has three classes (most likely the three ranks of the HBM stacks; nothing in an address tells which):
 *                          concurrent writes are fastest spread over two classes, reads inside one, and reads and writes in different
 *                          ones.  More chunks than needed are created, every chunk's class is MEASURED (a 0.2-ms probe kernel per chunk and
 *                          class), `in` (and `aux`) get chunks of one class, `out`'s chunks are arranged so that the eight XCDs' concurrent write
 *                          positions (XCD x walks the x-th eighth of `out`) are spread evenly over classes at every moment -- over the
 *                          two classes `in` is not in when out_bytes >= 3 * in_bytes, over all three otherwise -- the rest is
 *                          released.  While a pair is alive, calls whose buffers lie inside it launch under the whole-column tile map.
 *                          u32 W=7 unpack at 10 M blocks: 0.866-0.869 of the 8 TB/s, pack 0.854, where two hipMallocs give anything
 *                          from 0.78 (both buffers in one class) to 0.86.  Transient cost: a pool of twice the pair (at least 48 GiB, growing to three
 *                          times the pair where the first pool lacks a class) for a second or so; pairs below 8 GiB are allocated as FL_LAYOUT_SEPARATE (a handful of chunks: nothing to arrange);
 *                          FL_ERR_HIP with hipErrorNotSupported where the device has no virtual-memory management.
 *   FL_LAYOUT_PROBE        the candidates are allocated one after the other -- INTERLEAVED, SEPARATE, and ZONED where its slab still fits --
 *                          a bare read/write stream of in_bytes : out_bytes (no codec work; fl_stream.hpp) is timed on each for a few
 *                          launches on `stream`, the fastest pair is kept (a later candidate must win by more than 1 %, ZONED by more
 *                          than 2 %: it pins ~64 GiB), the others are freed.  SYNCHRONOUS (about 10 launches over the buffers per
 *                          candidate; `stream` must not be capturing), and the buffers' contents are unspecified afterwards.  A candidate
 *                          that cannot be allocated is skipped; pairs too small to time (< 4 MiB) are allocated SEPARATE.
 * in / aux / out receive in_bytes / aux_bytes / out_bytes bytes (256-byte aligned; aux_bytes may be 0: *aux = NULL, aux itself may then
 * be NULL); *handle owns the memory: fl_column_pair_free(handle) releases it (NULL is a no-op) after waiting for the work queued on its
 * device, whatever the layout (hipFree waits the same way), so it may follow launches on the pair's buffers at once.  layout_kept (may
 * be NULL) receives the layout of the returned pair, probe_gbps (may be NULL; FL_LAYOUT_COUNT entries, indexed by layout, the FL_LAYOUT_PROBE slot stays
 * 0) the probe's GB/s (0 = not measured).  This is what bench.py's --placement auto does: the figure it prints is one this header
 * alone reproduces.
 * (An INTERLEAVED pair's addresses are never handed out twice within a process: on this ROCm (7.2) an address range that is unmapped and
 * mapped again keeps translating to the FIRST chunks it held -- tools/exp_vmm remap -- so the library takes its ranges from a private,
 * monotonically growing part of the address space, 16 .. 112 TiB: a pair uses its own size plus its pool's there, once, so a process can
 * construct a few hundred large pairs; after that INTERLEAVED fails with FL_ERR_HIP (hipErrorOutOfMemory) and PROBE falls back to the plain
 * layouts.)
 */
enum { FL_LAYOUT_SEPARATE = 0, FL_LAYOUT_ZONED = 1, FL_LAYOUT_PROBE = 2, FL_LAYOUT_INTERLEAVED = 3, FL_LAYOUT_COUNT = 4 };
int fl_column_pair_alloc(size_t in_bytes, size_t aux_bytes, size_t out_bytes, int layout, void *stream,
                         void **in, void **aux, void **out, void **handle, int *layout_kept,
                         uint32_t *probe_gbps);
int fl_column_pair_free(void *handle);

/*
 * Mixed-width columns (BASELINE.json config 5): block b has its own width widths[b].
 * The reference has no multi-block API; this is its caller loop
 *     for b in blocks { T::unchecked_unpack(widths[b], &packed[off[b]..], &mut out[b*1024..]) }
 * (bitpacking.rs:109-129; pack: bitpacking.rs:76-96; loop shape of benches/bitpacking.rs:80-97)
 * moved on-device.  The surface is the one SURVEY.md 8(b) names: two DEVICE arrays,
 *     widths [n_blocks]  uint8   width of block b (<= T)
 *     offsets[n_blocks]  uint64  byte offset of block b's 128*widths[b] bytes in the packed column
 *                                (multiples of 16; back-to-back blocks give multiples of 128)
 * read by the kernel itself (fl_<ty>_unpack_widths / fl_<ty>_pack_widths below): one wavefront per
 * block, blocks in column order, ONE launch, no host pass over the column, no allocation, any
 * block count.  `packed_bytes` is the size of the packed column.  The kernel checks every block's
 * preconditions itself: a block whose width exceeds T, whose offset is not a multiple of 16, or whose
 * 128*widths[b] bytes do not lie inside [0, packed_bytes) is SKIPPED (nothing is read or written for
 * it) and its FL_DEVERR_* bit is ORed into *err_flag -- the device-side form of bitpacking.rs:93/126
 * unreachable!() and of the length debug_asserts (:78-80, :111-113).
 *
 * fl_widths_to_offsets builds the back-to-back offsets on the device: offsets[b] = sum_{i<b}
 * 128*widths[i] (exclusive prefix sum, three small launches on `stream`, no scratch memory),
 * *total_bytes (device uint64, may be NULL) = the packed column's size, FL_DEVERR_WIDTH ORed into
 * *err_flag if some width exceeds type_bits.
 */
int fl_widths_to_offsets(unsigned type_bits, const uint8_t *widths, size_t n_blocks,
                         uint64_t *offsets, uint64_t *total_bytes, uint32_t *err_flag,
                         void *stream);

/*
 * Convenience owner of the two device arrays for callers that hold the widths on the HOST:
 * create validates the widths (FL_ERR_WIDTH), uploads them to the current device, runs
 * fl_widths_to_offsets and reads back the packed size.  fl_<ty>_unpack_mixed / pack_mixed are
 * fl_<ty>_unpack_widths / pack_widths over the plan's arrays.  The plan must be used on the
 * device it was created on and destroyed by the caller.
 */
typedef struct fl_mixed_plan fl_mixed_plan;
int fl_mixed_plan_create(unsigned type_bits, const uint8_t *widths, size_t n_blocks,
                         fl_mixed_plan **plan);
void fl_mixed_plan_destroy(fl_mixed_plan *plan);
size_t fl_mixed_plan_n_blocks(const fl_mixed_plan *plan);
/* total packed bytes of the column = sum 128*widths[b] */
uint64_t fl_mixed_plan_packed_bytes(const fl_mixed_plan *plan);
/* device pointers to the plan's uint64 byte offsets / uint8 widths [n_blocks] (owned by the plan) */
const uint64_t *fl_mixed_plan_offsets(const fl_mixed_plan *plan);
const uint8_t *fl_mixed_plan_widths(const fl_mixed_plan *plan);

#define FL_DECLARE_TYPE(T, S)                                                                   \
    /* BitPacking::unchecked_pack (bitpacking.rs:30,76-96) -> pack::<W> (:65-74) */             \
    int fl_##S##_pack(unsigned width, const T *in, T *out, size_t n_blocks, void *stream);      \
    /* BitPacking::unchecked_unpack (bitpacking.rs:44,109-129) -> unpack::<W> (:98-107) */      \
    int fl_##S##_unpack(unsigned width, const T *in, T *out, size_t n_blocks, void *stream);    \
    /* BitPacking::unchecked_unpack_single (bitpacking.rs:58,181-200) -> unpack_single::<W>    \
     * (:132-179), batched: out[k] = value at element indices[k] of the column, where          \
     * indices[k] = block*1024 + index_in_block.  Out-of-range indices make the call return    \
     * FL_ERR_INDEX on the host tier; on the device tier they write 0 and OR FL_DEVERR_INDEX   \
     * into *err_flag (a device uint32, may be NULL). */                                       \
    int fl_##S##_unpack_single(unsigned width, const T *packed, size_t n_blocks,                \
                               const uint64_t *indices, size_t n_indices, T *out,               \
                               uint32_t *err_flag, void *stream);                               \
    /* FoR::for_pack::<W> (ffor.rs:5-9,24-36).  references[b*reference_stride] is block b's    \
     * scalar; reference_stride 0 broadcasts references[0]. */                                 \
    int fl_##S##_for_pack(unsigned width, const T *in, const T *references,                     \
                          size_t reference_stride, T *out, size_t n_blocks, void *stream);      \
    /* FoR::unfor_pack::<W> (ffor.rs:11-17,38-50) */                                            \
    int fl_##S##_unfor_pack(unsigned width, const T *in, const T *references,                   \
                            size_t reference_stride, T *out, size_t n_blocks, void *stream);    \
    /* Delta::delta (delta.rs:7,24-33); bases is [n_blocks][LANES] (128 bytes per block) */     \
    int fl_##S##_delta(const T *in, const T *bases, T *out, size_t n_blocks, void *stream);     \
    /* Delta::undelta (delta.rs:9,36-45) */                                                     \
    int fl_##S##_undelta(const T *in, const T *bases, T *out, size_t n_blocks, void *stream);   \
    /* Delta::undelta_pack::<W> (delta.rs:11-16,47-63); output stays in transposed order */     \
    int fl_##S##_undelta_pack(unsigned width, const T *in, const T *bases, T *out,              \
                              size_t n_blocks, void *stream);                                   \
    /* EXTENSIONS beyond the reference's methods; defined as the compositions  \
     * the reference's own test/bench perform (delta.rs:88-100, benches/delta.rs:20-27):               \
     *   undelta_pack_untranspose(W, pk, bases) == untranspose(undelta_pack::<W>(pk, bases))           \
     *   transpose_delta_pack(W, v, bases)      == pack::<W>(delta(transpose(v), bases))               \
     * i.e. decode straight to ORIGINAL order / encode straight from it, saving one 2x(1024*T/8)-byte  \
     * round trip per block. */                                                                       \
    int fl_##S##_undelta_pack_untranspose(unsigned width, const T *in, const T *bases, T *out,  \
                                          size_t n_blocks, void *stream);                       \
    int fl_##S##_transpose_delta_pack(unsigned width, const T *in, const T *bases, T *out,      \
                                      size_t n_blocks, void *stream);                           \
    /* EXTENSIONS, reductions over what the reference functions produce:           \
     *   unpack_block_sums: sums[b] = sum of the 1024 values unpack::<W> yields for block b           \
     *                      (wrapping uint64) without materialising them: 128*W bytes in, 8 out.       \
     *   block_min_max:     mins[b], maxs[b] over unpacked block b -- an encoder's inputs for FoR's    \
     *                      reference and width before for_pack::<W> (ffor.rs:24-36). */              \
    int fl_##S##_unpack_block_sums(unsigned width, const T *in, size_t n_blocks, uint64_t *sums,  \
                                   void *stream);                                               \
    int fl_##S##_block_min_max(const T *in, size_t n_blocks, T *mins, T *maxs, void *stream);    \
    /*   unpack_compare:    bit i of mask[b*32 .. b*32+32) = (unpack::<W>(block b)[i] <op> constant),  \
     *                      i in the unpacked (index) order: a selection vector straight from packed   \
     *                      data, 128*W bytes in, 128 bytes out per block.  op is an fl_cmp (any other    \
     *                      value: FL_ERR_INDEX). */       \
    int fl_##S##_unpack_compare(unsigned width, const T *in, int op, T constant, size_t n_blocks, \
                                uint32_t *mask, void *stream);                                  \
    /* Transpose::transpose (transpose.rs:5,11-15) */                                           \
    int fl_##S##_transpose(const T *in, T *out, size_t n_blocks, void *stream);                 \
    /* Transpose::untranspose (transpose.rs:6,17-22) */                                         \
    int fl_##S##_untranspose(const T *in, T *out, size_t n_blocks, void *stream);               \
    /* unchecked_unpack / unchecked_pack (bitpacking.rs:109-129, :76-96) looped over blocks with    \
     * per-block device widths[] / offsets[] (see "Mixed-width columns" above) */                  \
    int fl_##S##_unpack_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed,  \
                               size_t packed_bytes, T *out, size_t n_blocks, uint32_t *err_flag,  \
                               void *stream);                                                    \
    int fl_##S##_pack_widths(const uint8_t *widths, const uint64_t *offsets, const T *in,        \
                             T *packed, size_t packed_bytes, size_t n_blocks, uint32_t *err_flag, \
                             void *stream);                                                      \
    /* FoR's and Delta's bodies over such a column -- the reference's const-W methods called with block b's width, as its     \
     * callers do per chunk:  unfor_pack::<widths[b]> / for_pack::<widths[b]> (ffor.rs:24-50) with references[b*reference_stride] \
     * (stride 0 broadcasts references[0]);  undelta_pack::<widths[b]> (delta.rs:47-63) with bases[b][LANES], its output in   \
     * transposed order, and the two fused transpose extensions above.  Same per-block checks, same *err_flag. */             \
    int fl_##S##_unfor_pack_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed,  \
                                   size_t packed_bytes, const T *references, size_t reference_stride, \
                                   T *out, size_t n_blocks, uint32_t *err_flag, void *stream);        \
    int fl_##S##_for_pack_widths(const uint8_t *widths, const uint64_t *offsets, const T *in,         \
                                 const T *references, size_t reference_stride, T *packed,             \
                                 size_t packed_bytes, size_t n_blocks, uint32_t *err_flag,            \
                                 void *stream);                                                       \
    int fl_##S##_undelta_pack_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed, \
                                     size_t packed_bytes, const T *bases, T *out, size_t n_blocks,    \
                                     uint32_t *err_flag, void *stream);                               \
    int fl_##S##_undelta_pack_untranspose_widths(const uint8_t *widths, const uint64_t *offsets,      \
                                                 const T *packed, size_t packed_bytes, const T *bases, \
                                                 T *out, size_t n_blocks, uint32_t *err_flag,         \
                                                 void *stream);                                       \
    int fl_##S##_transpose_delta_pack_widths(const uint8_t *widths, const uint64_t *offsets,          \
                                             const T *in, const T *bases, T *packed,                  \
                                             size_t packed_bytes, size_t n_blocks, uint32_t *err_flag, \
                                             void *stream);                                           \
    /* EXTENSION, the step between block_min_max and for_pack_widths in an encoder:  widths[b] = number of  \
     * bits of maxs[b] - mins[b] (0 for a constant block) -- the smallest W for which for_pack::<W>(block b, mins[b])         \
     * (ffor.rs:24-36; masked to W bits by macros.rs:73) loses nothing.  The reference itself selects no widths. */           \
    int fl_##S##_for_widths(const T *mins, const T *maxs, size_t n_blocks, uint8_t *widths,          \
                            void *stream);                                                            \
    /* unchecked_unpack_single (bitpacking.rs:58,181-200) over such a column, batched: out[k] = element  \
     * indices[k] (= block*1024 + index_in_block) of the column; an index past the column, a width  \
     * > T or a block outside the packed column writes 0 and ORs its FL_DEVERR_* bit into *err_flag */ \
    int fl_##S##_unpack_single_widths(const uint8_t *widths, const uint64_t *offsets,            \
                                      const T *packed, size_t packed_bytes, size_t n_blocks,      \
                                      const uint64_t *indices, size_t n_indices, T *out,          \
                                      uint32_t *err_flag, void *stream);                          \
    /* MANY SMALL ARRAYS in one launch -- the shape of a columnar engine's chunks (Vortex: 64 Ki values = 64 blocks per   \
     * chunk), whose per-chunk loop over unchecked_unpack / unchecked_pack (bitpacking.rs:109-129, :76-96) is launch-bound  \
     * when every chunk is its own call.  Four DEVICE arrays of length n_arrays: packed[a] / out[a] are device pointers      \
     * (16-byte aligned) to array a's packed and unpacked blocks, widths[a] its width, n_blocks[a] its block count;          \
     * max_blocks (host) >= every n_blocks[a] sizes the grid.  An array with a width > T or a misaligned / NULL pointer is    \
     * skipped and FL_DEVERR_WIDTH / FL_DEVERR_ALIGN is ORed into *err_flag; an array with n_blocks[a] > max_blocks has only  \
     * its first max_blocks (rounded up to a workgroup's share, 4 to 64 blocks) blocks processed and raises FL_DEVERR_BOUNDS;     \
     * max_blocks itself may not exceed 2^30 (FL_ERR_INDEX). */                                \
    int fl_##S##_unpack_batch(const T *const *packed, T *const *out, const uint8_t *widths,       \
                              const uint32_t *n_blocks, size_t n_arrays, uint32_t max_blocks,     \
                              uint32_t *err_flag, void *stream);                                  \
    int fl_##S##_pack_batch(const T *const *in, T *const *packed, const uint8_t *widths,          \
                            const uint32_t *n_blocks, size_t n_arrays, uint32_t max_blocks,       \
                            uint32_t *err_flag, void *stream);                                    \
    /* ... with FoR's bodies (ffor.rs:24-50): references[a] (a DEVICE array, one scalar per ARRAY -- a chunk's frame of       \
     * reference) is added to / subtracted from every value of array a: unfor_pack::<W> / for_pack::<W> per block. */         \
    int fl_##S##_unfor_pack_batch(const T *const *packed, T *const *out, const uint8_t *widths,   \
                                  const T *references, const uint32_t *n_blocks, size_t n_arrays, \
                                  uint32_t max_blocks, uint32_t *err_flag, void *stream);         \
    int fl_##S##_for_pack_batch(const T *const *in, T *const *packed, const uint8_t *widths,      \
                                const T *references, const uint32_t *n_blocks, size_t n_arrays,   \
                                uint32_t max_blocks, uint32_t *err_flag, void *stream);           \
    /* ... with Delta's bodies: bases[a] is a device pointer to array a's bases, [n_blocks[a]][LANES] (128 bytes per block):   \
     * undelta_pack::<W> per block (delta.rs:47-63; output in transposed order, or -- untranspose != 0 -- straight in original  \
     * order: the fused extension above), and the fused encode pack::<W>(delta(transpose(in), bases)). */                       \
    int fl_##S##_undelta_pack_batch(const T *const *packed, const T *const *bases, T *const *out,  \
                                    const uint8_t *widths, const uint32_t *n_blocks, size_t n_arrays, \
                                    uint32_t max_blocks, int untranspose, uint32_t *err_flag,       \
                                    void *stream);                                                  \
    int fl_##S##_transpose_delta_pack_batch(const T *const *in, const T *const *bases,             \
                                            T *const *packed, const uint8_t *widths,                \
                                            const uint32_t *n_blocks, size_t n_arrays,              \
                                            uint32_t max_blocks, uint32_t *err_flag, void *stream); \
    /* the same over a mixed-width plan (see fl_mixed_plan) */                                     \
    int fl_##S##_unpack_mixed(const fl_mixed_plan *plan, const T *packed, T *out, void *stream); \
    int fl_##S##_pack_mixed(const fl_mixed_plan *plan, const T *in, T *packed, void *stream);    \
    /* ---- host-pointer tier: the trait methods' own slice arguments ---- */                   \
    int fl_##S##_pack_host(unsigned width, const T *in, T *out, size_t n_blocks);               \
    int fl_##S##_unpack_host(unsigned width, const T *in, T *out, size_t n_blocks);             \
    int fl_##S##_unpack_single_host(unsigned width, const T *packed, size_t n_blocks,           \
                                    uint64_t index, T *value);                                  \
    int fl_##S##_for_pack_host(unsigned width, const T *in, T reference, T *out,                \
                               size_t n_blocks);                                                \
    int fl_##S##_unfor_pack_host(unsigned width, const T *in, T reference, T *out,              \
                                 size_t n_blocks);                                              \
    int fl_##S##_delta_host(const T *in, const T *bases, T *out, size_t n_blocks);              \
    int fl_##S##_undelta_host(const T *in, const T *bases, T *out, size_t n_blocks);            \
    int fl_##S##_undelta_pack_host(unsigned width, const T *in, const T *bases, T *out,         \
                                   size_t n_blocks);                                            \
    int fl_##S##_transpose_host(const T *in, T *out, size_t n_blocks);                          \
    int fl_##S##_untranspose_host(const T *in, T *out, size_t n_blocks);

FL_DECLARE_TYPE(uint8_t, u8)
FL_DECLARE_TYPE(uint16_t, u16)
FL_DECLARE_TYPE(uint32_t, u32)
FL_DECLARE_TYPE(uint64_t, u64)

/*
 * EXTENSION: selection masks from FoR-packed columns, defined as the composition
 *     bit i of mask[b*32 .. b*32+32) = (unfor_pack::<W_b>(block b, references[b*reference_stride])[i] <op> constant)
 * (ffor.rs:38-50, wrapping_add; i in the unpacked index order, LSB first: the layout of fl_<ty>_unpack_compare; op an fl_cmp,
 * unsigned, any other value FL_ERR_INDEX; reference_stride 0 broadcasts references[0]).  W_b is `width` in the uniform form (`in`
 * holds n_blocks blocks of 128*width bytes, back to back) and widths[b] at offsets[b] in the mixed-width form, which runs the
 * per-block device checks of fl_<ty>_unfor_pack_widths: a failing block is skipped -- its 32 mask words are left untouched -- and its
 * FL_DEVERR_* bit is ORed into *err_flag.  A block's reference r and width W bound its values to the cyclic range [r, r + 2^W - 1]:
 * a block that range decides (every value satisfies the predicate, or none does) is answered from its metadata alone and its packed
 * bytes are never read.  A plain bit-packed column is filtered with one zero reference and reference_stride 0.
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list above is a pinned surface.)
 */
#define FL_DECLARE_FOR_COMPARE(T, S)                                                                      \
    int fl_##S##_unfor_compare(unsigned width, const T *in, const T *references, size_t reference_stride, \
                               int op, T constant, size_t n_blocks, uint32_t *mask, void *stream);       \
    int fl_##S##_unfor_compare_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed,   \
                                      size_t packed_bytes, const T *references, size_t reference_stride, \
                                      int op, T constant, size_t n_blocks, uint32_t *mask,               \
                                      uint32_t *err_flag, void *stream);

FL_DECLARE_FOR_COMPARE(uint8_t, u8)
FL_DECLARE_FOR_COMPARE(uint16_t, u16)
FL_DECLARE_FOR_COMPARE(uint32_t, u32)
FL_DECLARE_FOR_COMPARE(uint64_t, u64)

/*
 * EXTENSION: interval predicates chained through a mask -- WHERE ts BETWEEN a AND b AND status = 3 AND delta < 0 --
 * over the same columns, uniform or mixed width.  Defined as the composition (all arithmetic mod 2^T)
 *     v         = unfor_pack::<W_b>(block b, references[b*reference_stride])[i]                                  (ffor.rs:38-50)
 *     hit[b][i] = ((v - lo) mod 2^T) <= ((hi - lo) mod 2^T)                    -- the cyclic interval [lo, hi]
 *     FL_MASK_NEW: mask[b] = hit[b]   (mask_in ignored, may be NULL)
 *     FL_MASK_AND: mask[b] = mask_in[b] & hit[b]          FL_MASK_OR: mask[b] = mask_in[b] | hit[b]
 * lo <= hi is BETWEEN; lo > hi wraps and means v >= lo OR v <= hi; hi == lo - 1 matches every value.  Every unsigned fl_cmp
 * predicate is such an interval (or matches nothing), and so is every SIGNED one over the two's-complement bit patterns: x < k is
 * [2^(T-1), k - 1].  The complement of [lo, hi] is [hi + 1, lo - 1] unless the interval is full.  Masks have the layout of
 * fl_<ty>_unpack_compare: 32 words per block, bit i % 32 of word b*32 + i/32.  Every valid block's 128 mask bytes are always written.
 * `mask` may be the same pointer as `mask_in` (in place); ANY OTHER OVERLAP of the two is the caller's error.
 * A block is answered without reading its packed bytes when its reference and width decide it (the rule of fl_<ty>_unfor_compare),
 * when `combine` is AND and its mask_in is all zero, or when `combine` is OR and its mask_in is all ones.  The mixed-width form runs
 * the per-block device checks of fl_<ty>_unfor_compare_widths with the same contract -- a failing block is skipped, its FL_DEVERR_*
 * bit is ORed into *err_flag, its 32 mask words are left as they were -- so both can sit in one chain.
 * width > T is FL_ERR_WIDTH (also for an empty column); a `combine` outside the enum FL_ERR_INDEX; n_blocks == 0 FL_OK; mask_in ==
 * NULL with AND / OR, or any other required pointer NULL, FL_ERR_NULL (`in` / `packed` may be NULL only when no byte can be read:
 * width 0, or packed_bytes == 0); the packed column, `mask` and `mask_in` are 16-byte aligned (FL_ERR_ALIGN).
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list, the list of other functions and the other macros' symbol lists
 * are pinned surfaces.)
 */
typedef enum fl_mask_combine { FL_MASK_NEW = 0, FL_MASK_AND = 1, FL_MASK_OR = 2 } fl_mask_combine;

#define FL_DECLARE_FOR_COMPARE_RANGE(T, S)                                                                \
    int fl_##S##_unfor_compare_range(unsigned width, const T *in, const T *references, size_t reference_stride, \
                                     T lo, T hi, int combine, const uint32_t *mask_in /* NULL with FL_MASK_NEW */, \
                                     size_t n_blocks, uint32_t *mask, void *stream);                      \
    int fl_##S##_unfor_compare_range_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed, \
                                            size_t packed_bytes, const T *references, size_t reference_stride, \
                                            T lo, T hi, int combine, const uint32_t *mask_in /* NULL with FL_MASK_NEW */, \
                                            size_t n_blocks, uint32_t *mask, uint32_t *err_flag, void *stream);

FL_DECLARE_FOR_COMPARE_RANGE(uint8_t, u8)
FL_DECLARE_FOR_COMPARE_RANGE(uint16_t, u16)
FL_DECLARE_FOR_COMPARE_RANGE(uint32_t, u32)
FL_DECLARE_FOR_COMPARE_RANGE(uint64_t, u64)

/*
 * EXTENSION (SURVEY.md 8(f2) "unpack -> filter", 8(f4) "take"): decode only the rows a selection mask keeps.  For a FoR-packed
 * column, uniform or mixed width, and a mask in the layout the compare entry points write (32 uint32 words per block, bit i of
 * block b = bit i % 32 of word b*32 + i/32, i in the unpacked index order):
 *     out = concat over b ascending of [ unfor_pack::<W_b>(block b, references[b*reference_stride])[i]  for i ascending if bit i ]
 * (ffor.rs:38-50) -- the kept values, compacted, in column order.  A plain bit-packed column is selected with one zero reference and
 * reference_stride 0.  A Delta-packed column has fl_<ty>_undelta_select (below).  Two steps, both asynchronous on `stream`, no
 * allocation, no synchronisation:
 *   1. the mask-offsets call (type-independent): out_offsets[b] = number of mask bits set in blocks 0..b-1 (a device uint64 array, in
 *      ELEMENTS), *total (device uint64, may be NULL) = the number of kept values.  Three small launches, no scratch memory.
 *   2. fl_<ty>_unfor_select / fl_<ty>_unfor_select_widths: block b's kept values go to out[out_offsets[b] ..].  The count is taken from
 *      the block's own mask bits; a block whose run does not lie inside [0, out_len) is SKIPPED and FL_DEVERR_BOUNDS is ORed into
 *      *err_flag, so a wrong out_offsets array never writes outside `out`.  The mixed-width form runs the per-block device checks of
 *      fl_<ty>_unfor_pack_widths: a failing block is skipped, its output slots are left untouched, its FL_DEVERR_* bit is raised.
 *      A block whose mask is all zero is never read: no packed load, no store.
 * `out`, `mask` and the packed column are 16-byte aligned (FL_ERR_ALIGN); a block's own destination is only element-aligned.
 * A selection that keeps nothing has no output: `out` may be NULL when out_len is 0.
 * (Declared by macros of their own: FL_DECLARE_TYPE's per-type list and the list of other functions are pinned surfaces.)
 */
#define FL_DECLARE_MASK_OFFSETS(NAME)                                                                     \
    int fl_##NAME(const uint32_t *mask, size_t n_blocks, uint64_t *out_offsets, uint64_t *total, void *stream);
FL_DECLARE_MASK_OFFSETS(mask_offsets)

#define FL_DECLARE_SELECT(T, S)                                                                           \
    int fl_##S##_unfor_select(unsigned width, const T *in, const T *references, size_t reference_stride,  \
                              const uint32_t *mask, const uint64_t *out_offsets, T *out, size_t out_len,  \
                              size_t n_blocks, uint32_t *err_flag, void *stream);                         \
    int fl_##S##_unfor_select_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed,     \
                                     size_t packed_bytes, const T *references, size_t reference_stride,   \
                                     const uint32_t *mask, const uint64_t *out_offsets, T *out,           \
                                     size_t out_len, size_t n_blocks, uint32_t *err_flag, void *stream);

FL_DECLARE_SELECT(uint8_t, u8)
FL_DECLARE_SELECT(uint16_t, u16)
FL_DECLARE_SELECT(uint32_t, u32)
FL_DECLARE_SELECT(uint64_t, u64)

/*
 * EXTENSION (SURVEY.md 8(f2) "unpack -> filter" followed by a reduction): COUNT / SUM / MIN / MAX of a FoR-packed column, uniform or
 * mixed width, over the rows a selection mask keeps -- SELECT COUNT(*), SUM(y), MIN(y), MAX(y) WHERE <mask> -- without materialising
 * the kept rows.  With the mask in the layout the compare entry points write (32 uint32 words per block, bit i of block b = bit i % 32
 * of word b*32 + i/32, i in the unpacked index order):
 *     V_b   = [ unfor_pack::<W_b>(block b, references[b*reference_stride])[i]  for i if bit i of block b ]            (ffor.rs:38-50)
 *     agg_b = { count = |V_b|,  sum = the sum of V_b (values zero-extended to uint64, wrapping mod 2^64, as unpack_block_sums),
 *               min = min V_b,  max = max V_b   (unsigned, zero-extended to uint64) }
 * An empty V_b gives the IDENTITY {0, 0, UINT64_MAX, 0} of
 *     combine(a, b) = { a.count + b.count, a.sum + b.sum (wrapping), min(a.min, b.min), max(a.max, b.max) }.
 * mask == NULL keeps every row, and no mask is read.  reference_stride 0 broadcasts references[0]; one zero reference with stride 0
 * aggregates a plain bit-packed column.  A Delta-packed column has fl_<ty>_undelta_aggregate (below).  Two steps, both asynchronous on `stream`, no
 * allocation, no synchronisation:
 *   1. fl_<ty>_unfor_aggregate / fl_<ty>_unfor_aggregate_widths: block_aggs[b] = agg_b for EVERY block (a device array of n_blocks
 *      fl_block_aggregate, 32 bytes each) -- a result in its own right: per-chunk aggregates, zone maps.  A block whose mask is empty,
 *      or whose width is 0 (every value is its reference), is answered from its metadata: its packed bytes are never read.  The
 *      mixed-width form runs the per-block device checks of fl_<ty>_unfor_pack_widths: a failing block raises its FL_DEVERR_* bit in
 *      *err_flag and ITS SLOT RECEIVES THE IDENTITY.  This departs, on purpose, from the "left untouched" of the other mixed-width
 *      entry points: the slot feeds a reduction, and a skipped block must not inject stale memory into it.
 *   2. the aggregate-reduce call (type-independent): *result (a device fl_block_aggregate) = combine over block_aggs[0 .. n_blocks);
 *      n_blocks == 0 gives the identity.  Integer add, min and max are associative and commutative: the result is deterministic.
 *      Two small launches, no scratch memory.
 * width > T is FL_ERR_WIDTH (also for an empty column); `in` / `packed` may be NULL only when no byte can be read (width 0, or
 * packed_bytes == 0); `in` / `packed`, `mask` and `block_aggs` are 16-byte aligned (FL_ERR_ALIGN), and so is `result`.
 * block_aggs / result are declared `void *` -- pass a `fl_block_aggregate *` as it is -- so that every prototype of this header keeps to
 * the scalar types its language bindings map.
 * (Declared by macros of their own: FL_DECLARE_TYPE's per-type list and the list of other functions are pinned surfaces.)
 */
typedef struct { uint64_t count, sum, min, max; } fl_block_aggregate;          /* 32 bytes */

#define FL_DECLARE_AGGREGATE(T, S)                                                                        \
    int fl_##S##_unfor_aggregate(unsigned width, const T *in, const T *references, size_t reference_stride, \
                                 const uint32_t *mask /* may be NULL */, size_t n_blocks,                 \
                                 void *block_aggs, uint32_t *err_flag, void *stream);                     \
    int fl_##S##_unfor_aggregate_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed,  \
                                        size_t packed_bytes, const T *references, size_t reference_stride, \
                                        const uint32_t *mask /* may be NULL */, size_t n_blocks,          \
                                        void *block_aggs, uint32_t *err_flag, void *stream);

FL_DECLARE_AGGREGATE(uint8_t, u8)
FL_DECLARE_AGGREGATE(uint16_t, u16)
FL_DECLARE_AGGREGATE(uint32_t, u32)
FL_DECLARE_AGGREGATE(uint64_t, u64)

#define FL_DECLARE_AGGREGATE_REDUCE(NAME)                                                                 \
    int fl_##NAME(const void *block_aggs, size_t n_blocks, void *result, void *stream);
FL_DECLARE_AGGREGATE_REDUCE(aggregate_reduce)

/*
 * EXTENSION (GROUP BY on top of the aggregate above): COUNT / SUM / MIN / MAX of a FoR-packed VALUE column of type T grouped by a
 * FoR-packed KEY column of type u8 with the same n_blocks, over the rows a selection mask keeps -- SELECT k, COUNT(*), SUM(y), MIN(y),
 * MAX(y) WHERE <mask> GROUP BY k -- without materialising either column.  Both columns are uniform width (the first form) or both
 * mixed width (the _widths form); the mask has the layout the compare entry points write (32 uint32 words per block, bit i of block b
 * = bit i % 32 of word b*32 + i/32).  As a composition of reference functions:
 *     val_b[i] = unfor_pack::<W_b >(value block b, references    [b * reference_stride    ])[i]                       (ffor.rs:38-50)
 *     key_b[i] = unfor_pack::<KW_b>(key   block b, key_references[b * key_reference_stride])[i]                (u8, wrapping add)
 *     result[g] = combine over all (b, i) with mask bit (b, i) set and key_b[i] == g of {1, val, val, val}
 * with val = val_b[i] zero-extended to uint64, and combine and the identity {0, 0, UINT64_MAX, 0} exactly those of fl_block_aggregate
 * above.  `result` is ALWAYS 256 slots (a device array of 256 fl_block_aggregate, 8 KiB), one per possible u8 key: there is no
 * n_groups argument, so a key can never be out of range.  Every slot is written by every call; a group that does not occur, and every
 * group when n_blocks == 0, receives the identity.  mask == NULL keeps every row, and no mask is read; a reference stride of 0
 * broadcasts references[0] / key_references[0].  Integer add, min and max are associative and commutative: the result is
 * deterministic.  Asynchronous on `stream`, no allocation, no synchronisation, no scratch memory: a small launch writes the 256
 * identities, the kernel behind it folds its wavefronts' tables into them with 64-bit atomics.
 * A block whose mask is empty is never read; a key block of width 0 (a column sorted or clustered by key) is answered from its
 * reference, no key byte is read, and its value block is aggregated exactly as fl_<ty>_unfor_aggregate does (a value width of 0 reads
 * nothing at all).  The mixed-width form runs the per-block device checks of fl_<ty>_unfor_pack_widths on BOTH columns: a block that
 * fails either check raises its FL_DEVERR_* bit in *err_flag and contributes NOTHING; neither of its columns is read.
 * width > T or key_width > 8 is FL_ERR_WIDTH (also for an empty column); `result` is required by every call, the other pointers when
 * n_blocks > 0 (FL_ERR_NULL) -- `in` / `packed` / `keys` may be NULL only when no byte of it can be read (width 0, or its packed
 * bytes == 0); `in` / `packed`, `keys`, `mask` and `result` are 16-byte aligned (FL_ERR_ALIGN).
 * Out of scope: keys wider than u8 (a hash group-by), Delta columns, several value columns per launch, and the host tier.
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list and the list of other functions are pinned surfaces.)
 */
#define FL_DECLARE_AGGREGATE_BY(T, S)                                                                     \
    int fl_##S##_unfor_aggregate_by(unsigned width, const T *in, const T *references, size_t reference_stride, \
                                    unsigned key_width, const uint8_t *keys, const uint8_t *key_references, \
                                    size_t key_reference_stride, const uint32_t *mask /* may be NULL */,  \
                                    size_t n_blocks, void *result /* fl_block_aggregate[256] */,          \
                                    uint32_t *err_flag, void *stream);                                    \
    int fl_##S##_unfor_aggregate_by_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed, \
                                           size_t packed_bytes, const T *references, size_t reference_stride, \
                                           const uint8_t *key_widths, const uint64_t *key_offsets,        \
                                           const uint8_t *keys, size_t keys_bytes,                        \
                                           const uint8_t *key_references, size_t key_reference_stride,    \
                                           const uint32_t *mask /* may be NULL */, size_t n_blocks,       \
                                           void *result /* fl_block_aggregate[256] */,                    \
                                           uint32_t *err_flag, void *stream);

FL_DECLARE_AGGREGATE_BY(uint8_t, u8)
FL_DECLARE_AGGREGATE_BY(uint16_t, u16)
FL_DECLARE_AGGREGATE_BY(uint32_t, u32)
FL_DECLARE_AGGREGATE_BY(uint64_t, u64)

/*
 * EXTENSION: a predicate BETWEEN TWO COLUMNS -- WHERE commit_date < receipt_date, WHERE bid > ask, WHERE a = b --
 * over two FoR-packed columns of the SAME element type T and the same n_blocks, both uniform width (the first form; the two widths may
 * differ) or both mixed width (the _widths form), chained through a mask like fl_<ty>_unfor_compare_range.  Neither column is
 * materialised.  Defined as the composition (all arithmetic mod 2^T)
 *     va        = unfor_pack::<WA_b>(a block b, a_references[b*a_reference_stride])[i]                               (ffor.rs:38-50)
 *     vb        = unfor_pack::<WB_b>(b block b, b_references[b*b_reference_stride])[i]
 *     bias      = is_signed ? 2^(T-1) : 0
 *     hit[b][i] = ((va + bias) mod 2^T) <op> ((vb + bias) mod 2^T)             -- unsigned comparison, op an fl_cmp
 *     FL_MASK_NEW: mask[b] = hit[b]   (mask_in ignored, may be NULL)
 *     FL_MASK_AND: mask[b] = mask_in[b] & hit[b]          FL_MASK_OR: mask[b] = mask_in[b] | hit[b]
 * is_signed != 0 compares the two's-complement values.  Masks have the layout of fl_<ty>_unpack_compare: 32 words per block, bit
 * i % 32 of word b*32 + i/32.  Every valid block's 128 mask bytes are always written.  `mask` may be the same pointer as `mask_in`
 * (in place); ANY OTHER OVERLAP of the two is the caller's error.  A reference stride of 0 broadcasts references[0].
 * A block is answered without reading EITHER column's packed bytes when `combine` is AND and its mask_in is all zero, when `combine`
 * is OR and its mask_in is all ones, or when the two blocks' references and widths decide it: for the ordering ops when the hulls of
 * the two value ranges do not overlap (or touch in the one value that decides), for == / != when the two cyclic ranges are disjoint
 * or both widths are 0.  Otherwise only the columns of width >= 1 are read: a constant block against a packed block reads one block.
 * The mixed-width form runs the per-block device checks of fl_<ty>_unfor_pack_widths on BOTH columns: a block that fails either
 * check is skipped, its FL_DEVERR_* bits are ORed into *err_flag, its 32 mask words are left as they were (the contract of
 * fl_<ty>_unfor_compare_widths), and neither column is read.
 * Either width > T is FL_ERR_WIDTH (also for an empty column); an `op` or a `combine` outside its enum FL_ERR_INDEX; n_blocks == 0
 * FL_OK; mask_in == NULL with AND / OR, or any other required pointer NULL, FL_ERR_NULL (a column's packed pointer may be NULL only
 * when no byte of it can be read: its width is 0, or its packed bytes are 0); the packed columns, `mask` and `mask_in` are 16-byte
 * aligned (FL_ERR_ALIGN).
 * Out of scope: columns of different element types, arithmetic inside the predicate (a + b < k; an aggregate of a * b, a + b or a - b is
 * fl_<ty>_unfor_aggregate_columns), Delta columns, the host tier.
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list, the list of other functions and the other macros' symbol lists
 * are pinned surfaces.)
 */
#define FL_DECLARE_FOR_COMPARE_COLUMNS(T, S)                                                              \
    int fl_##S##_unfor_compare_columns(unsigned width_a, const T *a, const T *a_references, size_t a_reference_stride, \
                                       unsigned width_b, const T *b, const T *b_references, size_t b_reference_stride, \
                                       int op, int is_signed, int combine,                                \
                                       const uint32_t *mask_in /* NULL with FL_MASK_NEW */,               \
                                       size_t n_blocks, uint32_t *mask, void *stream);                    \
    int fl_##S##_unfor_compare_columns_widths(const uint8_t *a_widths, const uint64_t *a_offsets, const T *a_packed, \
                                              size_t a_packed_bytes, const T *a_references, size_t a_reference_stride, \
                                              const uint8_t *b_widths, const uint64_t *b_offsets, const T *b_packed, \
                                              size_t b_packed_bytes, const T *b_references, size_t b_reference_stride, \
                                              int op, int is_signed, int combine,                         \
                                              const uint32_t *mask_in /* NULL with FL_MASK_NEW */,        \
                                              size_t n_blocks, uint32_t *mask, uint32_t *err_flag, void *stream);

FL_DECLARE_FOR_COMPARE_COLUMNS(uint8_t, u8)
FL_DECLARE_FOR_COMPARE_COLUMNS(uint16_t, u16)
FL_DECLARE_FOR_COMPARE_COLUMNS(uint32_t, u32)
FL_DECLARE_FOR_COMPARE_COLUMNS(uint64_t, u64)

/*
 * EXTENSION: an aggregate of ARITHMETIC BETWEEN TWO COLUMNS -- SELECT SUM(price * discount), SUM(bid - ask),
 * MAX(a + b), a dot product -- over two FoR-packed columns of the SAME element type T and the same n_blocks, both uniform width (the
 * first form; the two widths may differ) or both mixed width (the _widths form), over the rows a selection mask keeps.  Neither
 * column is materialised.  Defined as the composition
 *     va      = unfor_pack::<WA_b>(a block b, a_references[b*a_reference_stride])[i]                                 (ffor.rs:38-50)
 *     vb      = unfor_pack::<WB_b>(b block b, b_references[b*b_reference_stride])[i]
 *     x[b][i] = (zext64(va) o zext64(vb)) mod 2^64          o = `expr`, an fl_expr: FL_EXPR_MUL a * b, FL_EXPR_ADD a + b, FL_EXPR_SUB a - b
 *     agg_b   = { count, sum of x (wrapping mod 2^64), min x, max x } over the i whose bit is set in block b of `mask`
 * with fl_block_aggregate, its identity {0, 0, UINT64_MAX, 0} for a block that keeps nothing, `combine` and the mask layout exactly
 * those of fl_<ty>_unfor_aggregate; mask == NULL keeps every row, and no mask is read.  The values are widened to 64 bits BEFORE the
 * operation: u8 / u16 / u32 products and sums are exact, u64 ones wrap.  A difference below zero is its two's-complement bit pattern,
 * so the SUM is right mod 2^64 (read it as int64_t); MIN AND MAX COMPARE THE PATTERNS AS UNSIGNED NUMBERS: every negative difference
 * lies above every non-negative one.  A reference stride of 0 broadcasts references[0]; one zero reference with stride 0 on both
 * sides gives the plain bit-packed product.
 * block_aggs[b] = agg_b for EVERY block (n_blocks fl_block_aggregate); the total is fl_aggregate_reduce over those slots, as for
 * fl_<ty>_unfor_aggregate.  A block whose mask is empty, or whose two widths are both 0 (every row holds ra o rb), is answered from
 * its metadata: neither column's packed bytes are read.  A column whose width is 0 in a block is never read there: a constant block
 * against a packed block reads one block.  The mixed-width form runs the per-block device checks of fl_<ty>_unfor_pack_widths on BOTH
 * columns: a block that fails either check raises its FL_DEVERR_* bits in *err_flag, reads neither column and ITS SLOT RECEIVES THE
 * IDENTITY (the contract of fl_<ty>_unfor_aggregate_widths: the slot feeds a reduction).
 * Either width > T is FL_ERR_WIDTH (also for an empty column); an `expr` outside fl_expr FL_ERR_INDEX; n_blocks == 0 FL_OK; a
 * required pointer NULL FL_ERR_NULL (a column's packed pointer may be NULL only when no byte of it can be read: its width is 0, or
 * its packed bytes are 0; `mask` may be NULL); the packed columns, `mask` and `block_aggs` are 16-byte aligned (FL_ERR_ALIGN).
 * Out of scope: signed (sign-extending) columns, columns of different element types, Delta columns, grouping, the host tier.
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list, the list of other functions and the other macros' symbol lists
 * are pinned surfaces.)
 */
typedef enum fl_expr { FL_EXPR_MUL = 0, FL_EXPR_ADD = 1, FL_EXPR_SUB = 2 } fl_expr;

#define FL_DECLARE_AGGREGATE_COLUMNS(T, S)                                                                \
    int fl_##S##_unfor_aggregate_columns(int expr, unsigned width_a, const T *a, const T *a_references,   \
                                         size_t a_reference_stride, unsigned width_b, const T *b,         \
                                         const T *b_references, size_t b_reference_stride,                \
                                         const uint32_t *mask /* may be NULL */, size_t n_blocks,         \
                                         void *block_aggs, uint32_t *err_flag, void *stream);             \
    int fl_##S##_unfor_aggregate_columns_widths(int expr, const uint8_t *a_widths, const uint64_t *a_offsets, const T *a_packed, \
                                                size_t a_packed_bytes, const T *a_references, size_t a_reference_stride, \
                                                const uint8_t *b_widths, const uint64_t *b_offsets, const T *b_packed, \
                                                size_t b_packed_bytes, const T *b_references, size_t b_reference_stride, \
                                                const uint32_t *mask /* may be NULL */, size_t n_blocks,  \
                                                void *block_aggs, uint32_t *err_flag, void *stream);

FL_DECLARE_AGGREGATE_COLUMNS(uint8_t, u8)
FL_DECLARE_AGGREGATE_COLUMNS(uint16_t, u16)
FL_DECLARE_AGGREGATE_COLUMNS(uint32_t, u32)
FL_DECLARE_AGGREGATE_COLUMNS(uint64_t, u64)

/*
 * EXTENSION: SET MEMBERSHIP chained through a mask -- WHERE shipmode IN ('MAIL', 'SHIP'), WHERE size IN (49, 14, 23),
 * a LIKE evaluated once on a dictionary and probed per row, the probe side of a semi-join -- over the same columns, uniform or mixed
 * width.  A member set is a WINDOW of the value domain plus a BITMAP: bit j of set_words (bit j % 32 of word j / 32), 0 <= j <
 * set_bits, says whether (set_lo + j) mod 2^T is a member.  0 <= set_bits <= min(2^T, 2^32); set_words holds ceil(set_bits / 32)
 * words; bits at positions >= set_bits of the last word are IGNORED (they need not be zero).  set_bits == 0 is the empty set: nothing
 * is a member, and set_words is not read (it may be NULL).  Defined as the composition (all arithmetic mod 2^T)
 *     v         = unfor_pack::<W_b>(block b, references[b*reference_stride])[i]                                  (ffor.rs:38-50)
 *     member(v) = (j := (v - set_lo) mod 2^T) < set_bits  &&  bit j of set_words
 *     hit[b][i] = member(v) XOR negate                                          -- negate 1: NOT IN
 *     FL_MASK_NEW: mask[b] = hit[b]   (mask_in ignored, may be NULL)
 *     FL_MASK_AND: mask[b] = mask_in[b] & hit[b]          FL_MASK_OR: mask[b] = mask_in[b] | hit[b]
 * A window that wraps past 2^T - 1 is as good as any other; a signed column's set is a window of its two's-complement bit patterns.
 * Masks have the layout of fl_<ty>_unpack_compare: 32 words per block, bit i % 32 of word b*32 + i/32.  Every valid block's 128 mask
 * bytes are always written.  `mask` may be the same pointer as `mask_in` (in place); ANY OTHER OVERLAP of the two is the caller's error.
 * A block is answered without reading its packed bytes when `combine` is AND and its mask_in is all zero, when `combine` is OR and
 * its mask_in is all ones, when its reference and width put all its values OUTSIDE the window (a miss; all hits under negate), or
 * when its width is 0 (one bitmap bit decides it).  A window of at most 2048 bits is held in registers (one 256-byte read per
 * wavefront); a larger one is probed in device memory, one cached 4-byte read per element inside the window.  The mixed-width form
 * runs the per-block device checks of fl_<ty>_unfor_compare_widths with the same contract -- a failing block is skipped, its
 * FL_DEVERR_* bit is ORed into *err_flag, its 32 mask words are left as they were -- so all of them can sit in one chain.
 * width > T is FL_ERR_WIDTH (also for an empty column); a `combine` outside the enum, a `negate` outside {0, 1} or set_bits above
 * min(2^T, 2^32) FL_ERR_INDEX; n_blocks == 0 FL_OK; mask_in == NULL with AND / OR, set_words == NULL with set_bits > 0, or any other
 * required pointer NULL, FL_ERR_NULL (`in` / `packed` may be NULL only when no byte can be read: width 0, or packed_bytes == 0); the
 * packed column, `mask`, `mask_in` and `set_words` are 16-byte aligned (FL_ERR_ALIGN).
 * The bitmap is built on the device from a key column by fl_<ty>_unfor_set_build below (a semi-join's build side).
 * Out of scope: windows above 2^32 bits, the host tier.
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list, the list of other functions and the other macros' symbol lists
 * are pinned surfaces.)
 */
#define FL_DECLARE_FOR_COMPARE_IN(T, S)                                                                   \
    int fl_##S##_unfor_compare_in(unsigned width, const T *in, const T *references, size_t reference_stride, \
                                  T set_lo, uint64_t set_bits, const uint32_t *set_words /* NULL with set_bits 0 */, \
                                  int negate, int combine, const uint32_t *mask_in /* NULL with FL_MASK_NEW */, \
                                  size_t n_blocks, uint32_t *mask, void *stream);                         \
    int fl_##S##_unfor_compare_in_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed, \
                                         size_t packed_bytes, const T *references, size_t reference_stride, \
                                         T set_lo, uint64_t set_bits, const uint32_t *set_words /* NULL with set_bits 0 */, \
                                         int negate, int combine, const uint32_t *mask_in /* NULL with FL_MASK_NEW */, \
                                         size_t n_blocks, uint32_t *mask, uint32_t *err_flag, void *stream);

FL_DECLARE_FOR_COMPARE_IN(uint8_t, u8)
FL_DECLARE_FOR_COMPARE_IN(uint16_t, u16)
FL_DECLARE_FOR_COMPARE_IN(uint32_t, u32)
FL_DECLARE_FOR_COMPARE_IN(uint64_t, u64)

/*
 * EXTENSION (the two aggregates above composed): COUNT / SUM / MIN / MAX of ARITHMETIC BETWEEN TWO COLUMNS, GROUPED BY A KEY --
 * SELECT k, SUM(price * discount) WHERE <mask> GROUP BY k (TPC-H Q1), revenue per status, a dot product per category -- over two
 * FoR-packed VALUE columns `a` and `b` of the SAME element type T and one FoR-packed KEY column of type u8, all three with the same
 * n_blocks, all three uniform width (the first form; the three widths may differ) or all three mixed width (the _widths form).  None
 * of the three columns is materialised.  Defined as the composition
 *     va  = unfor_pack::<WA_b>(a block b, a_references[b*a_reference_stride])[i]                                     (ffor.rs:38-50)
 *     vb  = unfor_pack::<WB_b>(b block b, b_references[b*b_reference_stride])[i]
 *     key = unfor_pack::<KW_b>(key block b, key_references[b*key_reference_stride])[i]                           (u8, wrapping add)
 *     x   = (zext64(va) o zext64(vb)) mod 2^64              o = `expr`, an fl_expr: FL_EXPR_MUL a * b, FL_EXPR_ADD a + b, FL_EXPR_SUB a - b
 *     result[g] = combine over all (b, i) with mask bit (b, i) set and key == g of {1, x, x, x}                      g = 0 .. 255
 * `combine`, the identity {0, 0, UINT64_MAX, 0}, the 256 fl_block_aggregate slots of `result`, the mask layout and mask == NULL are
 * exactly those of fl_<ty>_unfor_aggregate_by; the value semantics are exactly those of fl_<ty>_unfor_aggregate_columns: the values
 * are widened to 64 bits BEFORE the operation, so u8 / u16 / u32 results are exact and u64 ones wrap; a difference below zero is its
 * two's-complement 64-bit pattern (read the SUM as int64_t), and MIN AND MAX COMPARE THE PATTERNS AS UNSIGNED NUMBERS.  Every slot is
 * written by every call; a group that does not occur, and every group when n_blocks == 0, receives the identity.  A reference stride
 * of 0 broadcasts the column's references[0].  The result is deterministic.  Asynchronous on `stream`, no allocation, no
 * synchronisation, no scratch memory: the launches of fl_<ty>_unfor_aggregate_by.
 * A block whose mask is empty is never read; a key block of width 0 is answered from its reference, no key byte is read, and its two
 * value blocks are aggregated exactly as fl_<ty>_unfor_aggregate_columns does (two widths of 0 read nothing at all); a value column
 * whose width is 0 in a block is never read there.  The mixed-width form runs the per-block device checks of
 * fl_<ty>_unfor_pack_widths on ALL THREE columns: a block that fails any of them raises its FL_DEVERR_* bits in *err_flag and
 * contributes NOTHING; none of its columns is read.
 * width_a or width_b > T, or key_width > 8, is FL_ERR_WIDTH (also for an empty column); an `expr` outside fl_expr FL_ERR_INDEX;
 * `result` is required by every call, the other pointers when n_blocks > 0 (FL_ERR_NULL) -- a packed pointer may be NULL only when no
 * byte of it can be read (its width is 0, or its packed bytes are 0; `mask` may be NULL); the packed columns, `keys`, `mask` and
 * `result` are 16-byte aligned (FL_ERR_ALIGN).
 * SUM(a * (c - b)) per group for a constant c is c * SUM(a) - SUM(a * b): TPC-H Q1's sum_disc_price takes two launches, this one for
 * SUM(price * discount) and fl_<ty>_unfor_aggregate_by for SUM(price).
 * Out of scope: keys wider than u8, a second key column, more than one expression per launch, three-column products, constants inside
 * the expression, signed (sign-extending) columns, Delta columns, the host tier.
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list, the list of other functions and the other macros' symbol lists
 * are pinned surfaces.)
 */
#define FL_DECLARE_AGGREGATE_BY_COLUMNS(T, S)                                                             \
    int fl_##S##_unfor_aggregate_by_columns(int expr, unsigned width_a, const T *a, const T *a_references, \
                                            size_t a_reference_stride, unsigned width_b, const T *b,      \
                                            const T *b_references, size_t b_reference_stride,             \
                                            unsigned key_width, const uint8_t *keys, const uint8_t *key_references, \
                                            size_t key_reference_stride, const uint32_t *mask /* may be NULL */, \
                                            size_t n_blocks, void *result /* fl_block_aggregate[256] */,  \
                                            uint32_t *err_flag, void *stream);                            \
    int fl_##S##_unfor_aggregate_by_columns_widths(int expr, const uint8_t *a_widths, const uint64_t *a_offsets, const T *a_packed, \
                                                   size_t a_packed_bytes, const T *a_references, size_t a_reference_stride, \
                                                   const uint8_t *b_widths, const uint64_t *b_offsets, const T *b_packed, \
                                                   size_t b_packed_bytes, const T *b_references, size_t b_reference_stride, \
                                                   const uint8_t *key_widths, const uint64_t *key_offsets, \
                                                   const uint8_t *keys, size_t keys_bytes,                \
                                                   const uint8_t *key_references, size_t key_reference_stride, \
                                                   const uint32_t *mask /* may be NULL */, size_t n_blocks, \
                                                   void *result /* fl_block_aggregate[256] */,            \
                                                   uint32_t *err_flag, void *stream);

FL_DECLARE_AGGREGATE_BY_COLUMNS(uint8_t, u8)
FL_DECLARE_AGGREGATE_BY_COLUMNS(uint16_t, u16)
FL_DECLARE_AGGREGATE_BY_COLUMNS(uint32_t, u32)
FL_DECLARE_AGGREGATE_BY_COLUMNS(uint64_t, u64)

/*
 * EXTENSION: BUILD A MEMBER SET on the device -- the build side of the semi-join whose probe side is
 * fl_<ty>_unfor_compare_in: WHERE o_orderkey IN (SELECT l_orderkey FROM lineitem WHERE l_commitdate < l_receiptdate), every EXISTS.
 * The mask of any predicate chain on one table becomes a member set that filters another; both key columns stay packed.  Defined as
 * the composition (all arithmetic mod 2^T)
 *     for every block b, every i in 0..1023 with bit i of block b of `mask` set (mask == NULL: every i):
 *         v = unfor_pack::<W_b>(block b, references[b*reference_stride])[i]                                      (ffor.rs:38-50)
 *         j = (v - set_lo) mod 2^T
 *         if j < set_bits:  bit j of set_words |= 1;  inserted += 1          else:  outside += 1
 *     stats[0] += inserted;  stats[1] += outside                            -- stats: DEVICE uint64[2], may be NULL
 * set_lo, set_bits (0 <= set_bits <= min(2^T, 2^32)) and the layout of set_words (ceil(set_bits / 32) words, bit j % 32 of word j / 32)
 * are exactly those of fl_<ty>_unfor_compare_in: the output is passed to it as it stands.  THE CALL ORs AND ADDS, IT NEVER CLEARS: the
 * caller zeroes set_words and stats, or passes the result of an earlier call -- the union over several columns or masks is several
 * calls.  Bits at positions >= set_bits of the last word are never changed.  set_bits == 0 reads no packed byte, touches no word
 * (set_words may be NULL) and counts every kept row as outside.  OR and integer add commute: the result is bitwise reproducible.
 * `mask` has the layout of fl_<ty>_unpack_compare, 32 words per block.  A block whose mask is empty, a block whose reference and width
 * put all its values outside the window and a width-0 block (one bit) are answered without reading their packed bytes.  A window of at
 * most 65536 bits is built in a private bitmap per wavefront and ORed into set_words once per wavefront; a larger one takes one device
 * atomic per kept element inside the window.  The mixed-width form runs the per-block device checks of fl_<ty>_unfor_compare_widths:
 * a failing block is skipped, its FL_DEVERR_* bit is ORed into *err_flag, it contributes nothing to the bitmap or to stats.
 * width > T is FL_ERR_WIDTH (also for an empty column); set_bits above min(2^T, 2^32) FL_ERR_INDEX; n_blocks == 0 FL_OK (nothing is
 * touched); set_words == NULL with set_bits > 0, or any required column pointer NULL, FL_ERR_NULL (`in` / `packed` may be NULL only
 * when no byte can be read: width 0, or packed_bytes == 0); the packed column, `mask`, `set_words` and `stats` are 16-byte aligned
 * (FL_ERR_ALIGN).
 * Out of scope: Delta columns, the host tier, windows above 2^32 bits, counting bitmaps (multiplicities), keys of another type than
 * the probe column.
 */
#define FL_DECLARE_SET_BUILD(T, S)                                                                        \
    int fl_##S##_unfor_set_build(unsigned width, const T *in, const T *references, size_t reference_stride, \
                                 const uint32_t *mask /* NULL: every row */, size_t n_blocks,             \
                                 T set_lo, uint64_t set_bits, uint32_t *set_words /* NULL with set_bits 0 */, \
                                 uint64_t *stats /* may be NULL */, void *stream);                        \
    int fl_##S##_unfor_set_build_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed,  \
                                        size_t packed_bytes, const T *references, size_t reference_stride, \
                                        const uint32_t *mask /* NULL: every row */, size_t n_blocks,      \
                                        T set_lo, uint64_t set_bits, uint32_t *set_words /* NULL with set_bits 0 */, \
                                        uint64_t *stats /* may be NULL */, uint32_t *err_flag, void *stream);

FL_DECLARE_SET_BUILD(uint8_t, u8)
FL_DECLARE_SET_BUILD(uint16_t, u16)
FL_DECLARE_SET_BUILD(uint32_t, u32)
FL_DECLARE_SET_BUILD(uint64_t, u64)

/*
 * EXTENSION: GROUP BY A WIDE KEY inside a dense window of the key domain -- SELECT l_orderkey, SUM(l_quantity) ...
 * GROUP BY l_orderkey (TPC-H Q18, Q3), COUNT(*) GROUP BY o_custkey (Q13), SUM(revenue) GROUP BY l_suppkey (Q15), MIN(ps_supplycost)
 * GROUP BY ps_partkey (Q2): the grouped aggregate fl_<ty>_unfor_aggregate_by computes for a u8 key, for a key of the value column's own
 * type, with neither column materialised.  The value column and the key column have the SAME element type T and the same n_blocks (FoR
 * packing makes a narrow column cost its width, not its type: a u8-sized quantity next to a u32 key is a u32 column of width <= 8).
 * Defined as the composition (all key arithmetic mod 2^T)
 *     for every block b, every i in 0..1023 with bit i of block b of `mask` set (mask == NULL: every i):
 *         val = unfor_pack::<W_b >(value block b, references[b*reference_stride])[i]        zero-extended to uint64  (ffor.rs:38-50)
 *         key = unfor_pack::<KW_b>(key block b, key_references[b*key_reference_stride])[i]
 *         j   = (key - key_lo) mod 2^T
 *         if j < n_groups:  counts[j] += 1;  sums[j] += val (mod 2^64);  mins[j] = min(mins[j], val);  maxs[j] = max(maxs[j], val);
 *                           inside += 1
 *         else:             outside += 1
 *     stats[0] += inside;  stats[1] += outside                              -- stats: DEVICE uint64[2], may be NULL
 * counts, sums, mins and maxs are DEVICE uint64[n_groups] each, 0 <= n_groups <= min(2^T, 2^32); the window [key_lo, key_lo + n_groups
 * - 1] is cyclic, as fl_<ty>_unfor_set_build's.  THE CALL ACCUMULATES, IT NEVER CLEARS: the caller writes the identities 0 / 0 /
 * UINT64_MAX / 0 into the arrays, or passes the arrays of an earlier call -- several masks, several columns or several shards of one
 * table are several calls into one table.  An array passed as NULL is not maintained; when sums, mins and maxs are all NULL no packed
 * byte of the value column is read (its per-block checks still run); all four NULL is allowed, only stats is counted then.  n_groups
 * == 0 reads no packed byte, touches no array (they are not checked either) and counts every kept row as outside.  Integer add, min
 * and max commute: the result is bitwise reproducible.
 * `mask` has the layout of fl_<ty>_unpack_compare, 32 words per block.  A block whose mask is empty and a block whose key reference
 * and key width put all its keys outside the window are answered without reading either column; a key block of width 0 inside the
 * window folds the value block's aggregate into one slot without reading a key byte.  A window of at most 256 groups is aggregated in
 * a private table per wavefront and added to the arrays once per wavefront; a larger one takes one device atomic per kept element
 * inside the window and maintained array.  The mixed-width form runs the per-block device checks of fl_<ty>_unfor_compare_widths on
 * BOTH columns: a failing block is skipped, its FL_DEVERR_* bits are ORed into *err_flag, neither column is read and it contributes
 * nothing to the arrays or to stats.  The call is asynchronous on `stream`, allocates nothing and uses no scratch memory.
 * width or key_width > T is FL_ERR_WIDTH (also for an empty column); n_groups above min(2^T, 2^32) FL_ERR_INDEX; n_blocks == 0 FL_OK
 * (nothing is touched); any required column pointer NULL FL_ERR_NULL (`in` / `packed` / `keys` may be NULL only when no byte of it can
 * be read: width 0, or its packed bytes == 0); the packed columns, `mask`, the four arrays and `stats` are 16-byte aligned
 * (FL_ERR_ALIGN).
 * Out of scope: a value type different from the key type; sparse or hashed keys (a window is dense); windows above 2^32 groups; Delta
 * columns; the host tier; several value columns or an a o b expression per launch; a larger or workgroup-shared LDS table for mid-size
 * windows; combining a wavefront's equal keys before the atomic.
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list, the list of other functions and the other macros' symbol lists
 * are pinned surfaces.)
 */
#define FL_DECLARE_AGGREGATE_BY_WINDOW(T, S)                                                              \
    int fl_##S##_unfor_aggregate_by_window(unsigned width, const T *in, const T *references, size_t reference_stride, \
                                           unsigned key_width, const T *keys, const T *key_references,    \
                                           size_t key_reference_stride, const uint32_t *mask /* NULL: every row */, \
                                           size_t n_blocks, T key_lo, uint64_t n_groups,                  \
                                           uint64_t *counts /* may be NULL */, uint64_t *sums /* may be NULL */, \
                                           uint64_t *mins /* may be NULL */, uint64_t *maxs /* may be NULL */, \
                                           uint64_t *stats /* may be NULL */, void *stream);              \
    int fl_##S##_unfor_aggregate_by_window_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed, \
                                                  size_t packed_bytes, const T *references, size_t reference_stride, \
                                                  const uint8_t *key_widths, const uint64_t *key_offsets, \
                                                  const T *keys, size_t keys_bytes,                       \
                                                  const T *key_references, size_t key_reference_stride,   \
                                                  const uint32_t *mask /* NULL: every row */, size_t n_blocks, \
                                                  T key_lo, uint64_t n_groups,                            \
                                                  uint64_t *counts /* may be NULL */, uint64_t *sums /* may be NULL */, \
                                                  uint64_t *mins /* may be NULL */, uint64_t *maxs /* may be NULL */, \
                                                  uint64_t *stats /* may be NULL */, uint32_t *err_flag, void *stream);

FL_DECLARE_AGGREGATE_BY_WINDOW(uint8_t, u8)
FL_DECLARE_AGGREGATE_BY_WINDOW(uint16_t, u16)
FL_DECLARE_AGGREGATE_BY_WINDOW(uint32_t, u32)
FL_DECLARE_AGGREGATE_BY_WINDOW(uint64_t, u64)

/*
 * EXTENSION: LOOK UP A DIMENSION ATTRIBUTE through a packed key -- the probe side of a join that carries a payload:
 * SUM(revenue) GROUP BY n_name reached through l_suppkey or o_custkey (TPC-H Q5, Q7, Q8, Q10), GROUP BY d_year, p_brand through
 * lo_orderdate and lo_partkey (Star Schema Benchmark Q2 on), o_custkey through l_orderkey, ps_supplycost in Q9.  The window is the dense
 * one fl_<ty>_unfor_set_build, fl_<ty>_unfor_compare_in and fl_<ty>_unfor_aggregate_by_window share; the result is written AS A COLUMN
 * EVERY OPERATOR HERE CONSUMES UNCHANGED.  The payload type U is the key's own type T (fl_<ty>_unfor_lookup) or uint8_t
 * (fl_<ty>_unfor_lookup_u8; every element type has the same surface, so u8 declares it too: there it IS fl_u8_unfor_lookup, the
 * same kernel under its second name).  Defined as the composition (all key arithmetic mod 2^T)
 *     for every block b, every i in 0..1023:
 *         kept = mask == NULL or bit i of block b of `mask`
 *         key  = unfor_pack::<W_b>(key block b, references[b*reference_stride])[i]                                (ffor.rs:38-50)
 *         j    = (key - key_lo) mod 2^T
 *         hit  = kept and j < n_slots and (present == NULL or bit j of present)
 *         v[i] = hit ? table[j] : missing;   h[i] = hit
 *     out block b      = pack::<8*sizeof(U)>(v)          -- a permutation of v (bitpacking.rs); for U = uint8_t it is v itself
 *     hit_mask block b = h                               -- 32 words, the layout of fl_<ty>_unpack_compare; may be NULL
 *     stats[0] += #hit;  stats[1] += #(kept and not hit) -- stats: DEVICE uint64[2], may be NULL; it accumulates, as everywhere else
 * `table` is DEVICE U[n_slots], 0 <= n_slots <= min(2^T, 2^32); `present` has the layout of fl_<ty>_unfor_compare_in's set_words with
 * set_lo = key_lo and set_bits = n_slots (bits past n_slots are ignored) and may be NULL: every slot is present.  `out` is DEVICE
 * U[n_blocks * 1024].  A full-width bit-packed block is a pure permutation of its 1024 values, so
 *   - a uint8_t result is, as it stands, the FoR-packed u8 key column of fl_<ty>_unfor_aggregate_by and ..._by_columns (key_width = 8,
 *     one zero reference, stride 0);
 *   - a result of the key's own type is a valid input of every fl_<ty>_unfor_* entry point at width T with a zero reference -- a second
 *     lookup among them (l_orderkey -> o_custkey -> c_nationkey); fl_<ty>_unpack at width T gives it back in row order.
 * Every valid block's whole output block is always written, and its 128 mask bytes whenever hit_mask != NULL; `hit_mask` may be `mask`
 * itself (a block's incoming mask is read before its words are written).  n_slots == 0 reads no packed byte and no table byte, writes
 * `missing` everywhere and counts every kept row as a miss.
 * A block whose mask is empty and a block whose reference and width put all its keys outside the window are all `missing` without a
 * packed load or a gather; a width-0 block inside the window takes one table read.  A table of at most 8192 bytes is copied into LDS
 * once per wavefront; a larger one is gathered from device memory through one bounded buffer descriptor (default cache policy).  The
 * mixed-width form runs the per-block device checks of fl_<ty>_unfor_compare_widths: a failing block is skipped, its FL_DEVERR_* bit is
 * ORed into *err_flag, its `out` block and mask words are left untouched and it adds nothing to stats.  The call is asynchronous on
 * `stream`, allocates nothing and uses no scratch memory.
 * width > T is FL_ERR_WIDTH (also for an empty column); n_slots above min(2^T, 2^32), or n_slots * sizeof(U) >= 2^31, FL_ERR_INDEX;
 * n_blocks == 0 FL_OK (nothing is touched); table == NULL with n_slots > 0, out == NULL or any required column pointer NULL FL_ERR_NULL
 * (`in` / `packed` may be NULL only when no byte of it can be read: width 0, or packed_bytes == 0); the packed column, `mask`,
 * `hit_mask`, `present`, `table`, `out` and `stats` are 16-byte aligned (FL_ERR_ALIGN).
 * Out of scope: payload types other than T and uint8_t; several tables per launch; sparse or hashed keys (a window is dense); Delta
 * columns; the host tier; tables of 2^31 bytes or more.  (The fused GROUP BY through a uint8_t lookup, with no code column and no hit
 * mask written, is fl_<ty>_unfor_aggregate_by_lookup below.)
 * (Declared by two macros of their own: FL_DECLARE_TYPE's per-type list, the list of other functions and the other macros' symbol
 * lists are pinned surfaces.)
 */
#define FL_DECLARE_LOOKUP(T, S)                                                                           \
    int fl_##S##_unfor_lookup(unsigned width, const T *in, const T *references, size_t reference_stride,  \
                              const uint32_t *mask /* NULL: every row */, size_t n_blocks,                \
                              T key_lo, uint64_t n_slots, const T *table /* NULL with n_slots 0 */,       \
                              const uint32_t *present /* may be NULL */, T missing, T *out,               \
                              uint32_t *hit_mask /* may be NULL, may be mask */,                          \
                              uint64_t *stats /* may be NULL */, void *stream);                           \
    int fl_##S##_unfor_lookup_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed,     \
                                     size_t packed_bytes, const T *references, size_t reference_stride,   \
                                     const uint32_t *mask /* NULL: every row */, size_t n_blocks,         \
                                     T key_lo, uint64_t n_slots, const T *table /* NULL with n_slots 0 */, \
                                     const uint32_t *present /* may be NULL */, T missing, T *out,        \
                                     uint32_t *hit_mask /* may be NULL, may be mask */,                   \
                                     uint64_t *stats /* may be NULL */, uint32_t *err_flag, void *stream);

FL_DECLARE_LOOKUP(uint8_t, u8)
FL_DECLARE_LOOKUP(uint16_t, u16)
FL_DECLARE_LOOKUP(uint32_t, u32)
FL_DECLARE_LOOKUP(uint64_t, u64)

#define FL_DECLARE_LOOKUP_U8(T, S)                                                                        \
    int fl_##S##_unfor_lookup_u8(unsigned width, const T *in, const T *references, size_t reference_stride, \
                                 const uint32_t *mask /* NULL: every row */, size_t n_blocks,             \
                                 T key_lo, uint64_t n_slots, const uint8_t *table /* NULL with n_slots 0 */, \
                                 const uint32_t *present /* may be NULL */, uint8_t missing, uint8_t *out, \
                                 uint32_t *hit_mask /* may be NULL, may be mask */,                       \
                                 uint64_t *stats /* may be NULL */, void *stream);                        \
    int fl_##S##_unfor_lookup_u8_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed,  \
                                        size_t packed_bytes, const T *references, size_t reference_stride, \
                                        const uint32_t *mask /* NULL: every row */, size_t n_blocks,      \
                                        T key_lo, uint64_t n_slots, const uint8_t *table /* NULL with n_slots 0 */, \
                                        const uint32_t *present /* may be NULL */, uint8_t missing, uint8_t *out, \
                                        uint32_t *hit_mask /* may be NULL, may be mask */,                \
                                        uint64_t *stats /* may be NULL */, uint32_t *err_flag, void *stream);

FL_DECLARE_LOOKUP_U8(uint8_t, u8)
FL_DECLARE_LOOKUP_U8(uint16_t, u16)
FL_DECLARE_LOOKUP_U8(uint32_t, u32)
FL_DECLARE_LOOKUP_U8(uint64_t, u64)

/*
 * EXTENSION: GROUP BY A DIMENSION ATTRIBUTE, FUSED -- fl_<ty>_unfor_lookup_u8 and fl_<ty>_unfor_aggregate_by in one
 * pass: SUM(revenue) GROUP BY n_name reached through l_suppkey (TPC-H Q5, Q7, Q8, Q10), GROUP BY d_year, p_brand through lo_orderdate
 * and lo_partkey (Star Schema Benchmark Q2 on), with NO per-row output: no code column, no hit mask.  The value column and the key
 * column have the SAME element type T and the same n_blocks, as in fl_<ty>_unfor_aggregate_by_window.  Defined as the composition (all
 * key arithmetic mod 2^T)
 *     result[g] = identity {0, 0, UINT64_MAX, 0}                 for g = 0..255   (every slot written by every call)
 *     for every block b, every i in 0..1023 with bit i of block b of `mask` set (mask == NULL: every i):
 *         val = unfor_pack::<W_b >(value block b, references[b*reference_stride])[i]        zero-extended to uint64  (ffor.rs:38-50)
 *         key = unfor_pack::<KW_b>(key block b, key_references[b*key_reference_stride])[i]
 *         j   = (key - key_lo) mod 2^T
 *         hit = j < n_slots and (present == NULL or bit j of present)
 *         hit:  g = table[j];  result[g] = combine(result[g], {1, val, val, val});  hits += 1
 *         else: misses += 1
 *     stats[0] += hits;  stats[1] += misses        -- stats: DEVICE uint64[2], may be NULL; it accumulates, as everywhere else
 * `table` is DEVICE uint8_t[n_slots], 0 <= n_slots <= min(2^T, 2^32) and n_slots < 2^31; `present` has the layout of
 * fl_<ty>_unfor_lookup's (bits past n_slots are ignored) and may be NULL: every slot is present.  `result`, combine, the identity and
 * the mask layout are exactly those of fl_<ty>_unfor_aggregate_by: 256 fl_block_aggregate, written by every call.  The call equals,
 * bit for bit in `result` and in `stats`, fl_<ty>_unfor_lookup_u8[_widths] into a temporary with its hit mask followed by
 * fl_<ty>_unfor_aggregate_by[_widths] with that temporary as the full-width u8 key column and mask = the hits.  Integer add, min and max
 * commute: the result is bitwise reproducible.
 * A block whose mask is empty reads nothing; a block whose key reference and key width put all its keys outside the window (n_slots
 * == 0 among them) reads neither column and no table byte and counts its kept rows as misses; a key block of width 0 inside the window
 * takes one table read (and at most one `present` bit): an absent slot counts its kept rows as misses without reading the value block,
 * a present one folds the value block's aggregate into group table[c] without reading a key byte.  Every other block decodes both
 * columns and gathers one table byte per kept row inside the window through one bounded buffer descriptor (default cache policy; there
 * is no LDS copy of the table: the LDS holds the 256 groups).  The mixed-width form runs the per-block device checks of
 * fl_<ty>_unfor_compare_widths on BOTH columns: a failing block is skipped, its FL_DEVERR_* bits are ORed into *err_flag, neither
 * column is read and it contributes nothing to `result` or to stats.  The call is asynchronous on `stream`, allocates nothing and uses
 * no scratch memory.
 * width or key_width > T is FL_ERR_WIDTH (also for an empty column); n_slots above min(2^T, 2^32), or n_slots >= 2^31, FL_ERR_INDEX;
 * result == NULL, table == NULL with n_slots > 0 or any required column pointer NULL FL_ERR_NULL (`in` / `packed` / `keys` may be NULL
 * only when no byte of it can be read: width 0, or its packed bytes == 0); the packed columns, `mask`, `present`, `table`, `result` and
 * `stats` are 16-byte aligned (FL_ERR_ALIGN); n_blocks == 0 is FL_OK: `result` receives the 256 identities, as
 * fl_<ty>_unfor_aggregate_by's, and stats is untouched.
 * Out of scope: a value type different from the key type; payloads wider than uint8_t or more than 256 groups
 * (fl_<ty>_unfor_aggregate_by_window after a T-payload lookup serves those); several tables, or an a o b expression, per launch; an LDS
 * copy of the dimension table; sparse or hashed keys; Delta columns; the host tier; tables of 2^31 bytes or more.
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list, the list of other functions and the other macros' symbol lists
 * are pinned surfaces.)
 */
#define FL_DECLARE_AGGREGATE_BY_LOOKUP(T, S)                                                              \
    int fl_##S##_unfor_aggregate_by_lookup(unsigned width, const T *in, const T *references, size_t reference_stride, \
                                           unsigned key_width, const T *keys, const T *key_references,    \
                                           size_t key_reference_stride, const uint32_t *mask /* NULL: every row */, \
                                           size_t n_blocks, T key_lo, uint64_t n_slots,                   \
                                           const uint8_t *table /* NULL with n_slots 0 */,                \
                                           const uint32_t *present /* may be NULL */,                     \
                                           void *result /* fl_block_aggregate[256] */,                    \
                                           uint64_t *stats /* may be NULL */, uint32_t *err_flag, void *stream); \
    int fl_##S##_unfor_aggregate_by_lookup_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed, \
                                                  size_t packed_bytes, const T *references, size_t reference_stride, \
                                                  const uint8_t *key_widths, const uint64_t *key_offsets, \
                                                  const T *keys, size_t keys_bytes,                       \
                                                  const T *key_references, size_t key_reference_stride,   \
                                                  const uint32_t *mask /* NULL: every row */, size_t n_blocks, \
                                                  T key_lo, uint64_t n_slots,                             \
                                                  const uint8_t *table /* NULL with n_slots 0 */,         \
                                                  const uint32_t *present /* may be NULL */,              \
                                                  void *result /* fl_block_aggregate[256] */,             \
                                                  uint64_t *stats /* may be NULL */, uint32_t *err_flag, void *stream);

FL_DECLARE_AGGREGATE_BY_LOOKUP(uint8_t, u8)
FL_DECLARE_AGGREGATE_BY_LOOKUP(uint16_t, u16)
FL_DECLARE_AGGREGATE_BY_LOOKUP(uint32_t, u32)
FL_DECLARE_AGGREGATE_BY_LOOKUP(uint64_t, u64)

/*
 * EXTENSION: INTERVAL PREDICATES ON DELTA-PACKED COLUMNS -- WHERE l_shipdate BETWEEN a AND b on the sorted or nearly
 * sorted columns (dates, timestamps, clustered keys) a FastLanes writer stores Delta-coded, with no decoded column written or read back.
 * Defined as the composition (all arithmetic mod 2^T)
 *     v[b]      = untranspose(undelta_pack::<W_b>(block b, bases[b*LANES .. b*LANES + LANES]))    (delta.rs:47-63, transpose.rs:17-22)
 *     hit[b][i] = ((v[b][i] - lo) mod 2^T) <= ((hi - lo) mod 2^T)              -- the cyclic interval [lo, hi]
 *     FL_MASK_NEW: mask[b] = hit[b]   (mask_in ignored, may be NULL)
 *     FL_MASK_AND: mask[b] = mask_in[b] & hit[b]          FL_MASK_OR: mask[b] = mask_in[b] | hit[b]
 * i is the ORIGINAL row (the order fl_<ty>_undelta_pack_untranspose writes); the masks, the interval, `combine` and the in-place rule
 * (`mask` may be `mask_in` itself, any other overlap is the caller's error) are exactly those of fl_<ty>_unfor_compare_range, so the
 * result heads or joins any chain of the FoR consumers.  `bases` holds LANES = 1024 / T elements per block (128 bytes), as for
 * fl_<ty>_undelta_pack.  Every valid block's 128 mask bytes are always written.
 * A block is answered without reading its packed bytes when `combine` is AND and its mask_in is all zero or `combine` is OR and its
 * mask_in is all ones; when its bases and width decide it -- with c_l = (base_l - lo) mod 2^T, s = (hi - lo) mod 2^T and reach = T *
 * (2^W - 1): every c_l <= s and max c_l + reach <= s (all rows hit), or every c_l > s and max c_l + reach <= 2^T - 1 (none does); and
 * when its width is 0 (each lane's T rows repeat its base).  On a sorted column that is almost every block.  The mixed-width form runs
 * the per-block device checks of fl_<ty>_unfor_compare_widths with the same contract: a failing block is skipped, its FL_DEVERR_* bit
 * is ORed into *err_flag, its 32 mask words are left as they were.  Asynchronous on `stream`; allocates nothing, uses no scratch memory.
 * width > T is FL_ERR_WIDTH (also for an empty column); a `combine` outside the enum FL_ERR_INDEX; n_blocks == 0 FL_OK; mask_in ==
 * NULL with AND / OR, or any other required pointer NULL, FL_ERR_NULL (`in` / `packed` may be NULL only when no byte can be read:
 * width 0, or packed_bytes == 0); the packed column, `bases`, `mask` and `mask_in` are 16-byte aligned (FL_ERR_ALIGN).
 * Out of scope: masks in transposed order; the grouped Delta aggregates (fl_<ty>_undelta_aggregate and fl_<ty>_undelta_select, below,
 * aggregate and materialise one Delta column under such a mask); the host tier.
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list, the list of other functions and the other macros' symbol lists
 * are pinned surfaces.)
 */
#define FL_DECLARE_DELTA_COMPARE_RANGE(T, S)                                                              \
    int fl_##S##_undelta_compare_range(unsigned width, const T *in, const T *bases, T lo, T hi, int combine, \
                                       const uint32_t *mask_in /* NULL with FL_MASK_NEW */, size_t n_blocks, \
                                       uint32_t *mask, void *stream);                                     \
    int fl_##S##_undelta_compare_range_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed, \
                                              size_t packed_bytes, const T *bases, T lo, T hi, int combine, \
                                              const uint32_t *mask_in /* NULL with FL_MASK_NEW */, size_t n_blocks, \
                                              uint32_t *mask, uint32_t *err_flag, void *stream);

FL_DECLARE_DELTA_COMPARE_RANGE(uint8_t, u8)
FL_DECLARE_DELTA_COMPARE_RANGE(uint16_t, u16)
FL_DECLARE_DELTA_COMPARE_RANGE(uint32_t, u32)
FL_DECLARE_DELTA_COMPARE_RANGE(uint64_t, u64)

/*
 * EXTENSION: COUNT / SUM / MIN / MAX OF A DELTA-PACKED COLUMN, uniform or mixed width, over the rows a selection mask
 * keeps -- SELECT COUNT(*), MIN(ts), MAX(ts), SUM(ts) WHERE sensor = 3 AND ts BETWEEN a AND b on the sorted or nearly sorted columns a
 * FastLanes writer stores Delta-coded, and their per-block zone maps -- with no decoded column written or read back.  Defined as the
 * composition (arithmetic mod 2^T unless stated)
 *     v[b]  = untranspose(undelta_pack::<W_b>(block b, bases[b*LANES .. b*LANES + LANES]))        (delta.rs:47-63, transpose.rs:17-22)
 *     V_b   = [ v[b][i]  for i if bit i of block b of mask ]          mask == NULL: every i, and no mask is read
 *     agg_b = { count = |V_b|, sum = sum of V_b zero-extended to u64 (wrapping mod 2^64), min = min V_b, max = max V_b }
 *             nothing kept: the identity {0, 0, UINT64_MAX, 0}
 * The mask is the one every compare entry point writes and fl_<ty>_undelta_compare_range produces: 32 words per block, bit i = the
 * ORIGINAL row i, LSB first.  block_aggs[b] = agg_b for EVERY block (fl_block_aggregate, 32 bytes each); the reduction to one result is
 * fl_aggregate_reduce, and everything about slots, identity and determinism is fl_<ty>_unfor_aggregate's.  `bases` holds LANES =
 * 1024 / T elements per block (128 bytes), as for fl_<ty>_undelta_pack.
 * A block whose mask is empty, and a block of width 0 (each lane's T rows repeat its base: count = sum of p_l, sum = sum of p_l * base_l
 * with p_l the kept rows of lane l, min / max over the lanes with p_l > 0), read no packed byte.  The mixed-width form runs the per-block
 * device checks of fl_<ty>_unfor_pack_widths: a failing block raises its FL_DEVERR_* bit in *err_flag and ITS SLOT RECEIVES THE IDENTITY
 * (the aggregate's contract, not the compare's "left untouched").  err_flag follows fl_<ty>_unfor_aggregate[_widths]' rule.  Device
 * tier, asynchronous on `stream`; allocates nothing, uses no scratch memory.
 * width > T is FL_ERR_WIDTH (also for an empty column); n_blocks == 0 FL_OK; a required pointer NULL FL_ERR_NULL (`bases` is required;
 * `in` / `packed` may be NULL only when no byte can be read: width 0, or packed_bytes == 0); the packed column, `bases`, `mask` and
 * `block_aggs` are 16-byte aligned (FL_ERR_ALIGN).
 * Out of scope: grouped or two-column Delta aggregates, masks in transposed order, signed columns, the host tier (the Delta form of
 * select is fl_<ty>_undelta_select, below).
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list, the list of other functions and the other macros' symbol lists
 * are pinned surfaces.)
 */
#define FL_DECLARE_DELTA_AGGREGATE(T, S)                                                                  \
    int fl_##S##_undelta_aggregate(unsigned width, const T *in, const T *bases,                           \
                                   const uint32_t *mask /* may be NULL */, size_t n_blocks,               \
                                   void *block_aggs, uint32_t *err_flag, void *stream);                   \
    int fl_##S##_undelta_aggregate_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed, \
                                          size_t packed_bytes, const T *bases,                            \
                                          const uint32_t *mask /* may be NULL */, size_t n_blocks,        \
                                          void *block_aggs, uint32_t *err_flag, void *stream);

FL_DECLARE_DELTA_AGGREGATE(uint8_t, u8)
FL_DECLARE_DELTA_AGGREGATE(uint16_t, u16)
FL_DECLARE_DELTA_AGGREGATE(uint32_t, u32)
FL_DECLARE_DELTA_AGGREGATE(uint64_t, u64)

/*
 * EXTENSION (SURVEY.md 8(f2) "unpack -> filter", 8(f4) "take"): DECODE ONLY THE ROWS A SELECTION MASK KEEPS OF A DELTA-PACKED COLUMN,
 * uniform or mixed width -- SELECT l_shipdate WHERE <chain of predicates> on the sorted or nearly sorted columns a FastLanes writer
 * stores Delta-coded -- with no full-width decoded column written or read back.  Defined as the composition (arithmetic mod 2^T)
 *     v[b] = untranspose(undelta_pack::<W_b>(block b, bases[b*LANES .. b*LANES + LANES]))         (delta.rs:47-63, transpose.rs:17-22)
 *     out  = concat over b ascending of [ v[b][i]  for i ascending if bit i of block b of mask ]
 * -- the kept values, compacted, in ORIGINAL row order.  The mask is the one every compare entry point writes and
 * fl_<ty>_undelta_compare_range produces: 32 words per block, bit i = the ORIGINAL row i, LSB first.  `bases` holds LANES = 1024 / T
 * elements per block (128 bytes), as for fl_<ty>_undelta_pack.  The two steps are fl_<ty>_unfor_select's: fl_mask_offsets gives
 * out_offsets / *total (per-block popcounts do not depend on the row order), then block b's kept values go to out[out_offsets[b] ..].
 * Everything else is fl_<ty>_unfor_select's contract too: the count is taken from the block's own mask bits; a block whose run does not
 * lie inside [0, out_len) is SKIPPED and FL_DEVERR_BOUNDS is ORed into *err_flag (`err_flag` serves the uniform form too); the
 * mixed-width form runs the per-block device checks of fl_<ty>_unfor_pack_widths, and a failing block is skipped, its output slots left
 * untouched, its FL_DEVERR_* bit raised.  A block whose mask is all zero reads nothing and stores nothing; a block of width 0 (each
 * lane's T rows repeat its base) reads no packed byte.  Device tier, asynchronous on `stream`; allocates nothing, uses no scratch memory.
 * width > T is FL_ERR_WIDTH (also for an empty column); n_blocks == 0 FL_OK; a required pointer NULL FL_ERR_NULL (`bases`, `mask` and
 * `out_offsets` are required; `in` / `packed` may be NULL only when no byte can be read: width 0, or packed_bytes == 0; `out` may be
 * NULL when out_len is 0: a selection that keeps nothing has no output); the packed column, `bases`, `mask` and `out` are 16-byte
 * aligned (FL_ERR_ALIGN); a block's own destination is only element-aligned.
 * Out of scope: masks in transposed order, signed columns (the bit patterns are the same), the host tier.
 * (Declared by a macro of its own: FL_DECLARE_TYPE's per-type list, the list of other functions and the other macros' symbol lists
 * are pinned surfaces.)
 */
#define FL_DECLARE_DELTA_SELECT(T, S)                                                                     \
    int fl_##S##_undelta_select(unsigned width, const T *in, const T *bases,                              \
                                const uint32_t *mask, const uint64_t *out_offsets, T *out, size_t out_len, \
                                size_t n_blocks, uint32_t *err_flag, void *stream);                       \
    int fl_##S##_undelta_select_widths(const uint8_t *widths, const uint64_t *offsets, const T *packed,   \
                                       size_t packed_bytes, const T *bases, const uint32_t *mask,         \
                                       const uint64_t *out_offsets, T *out, size_t out_len,               \
                                       size_t n_blocks, uint32_t *err_flag, void *stream);

FL_DECLARE_DELTA_SELECT(uint8_t, u8)
FL_DECLARE_DELTA_SELECT(uint16_t, u16)
FL_DECLARE_DELTA_SELECT(uint32_t, u32)
FL_DECLARE_DELTA_SELECT(uint64_t, u64)

#ifdef __cplusplus
}
#endif
#endif /* FASTLANES_AMD_H */
