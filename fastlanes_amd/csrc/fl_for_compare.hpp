// fl_for_compare.hpp -- unfor_compare: a selection mask straight from a FoR-packed column, uniform or mixed width.
// EXTENSION, defined as a composition of reference functions:
//     bit i of mask[b*32 .. b*32+32) = (unfor_pack::<W_b>(block b, references[b * ref_stride])[i] <op> constant)
// (ffor.rs:38-50; i in the unpacked index order, LSB first, 32 words per block: unpack_compare's layout, fl_consume.hpp).
// The wave-per-block machinery of fl_widths.hpp (one wavefront per block, runtime width, the LDS image, WaveBlock::funnel), through
// the steps fl_for_block.hpp shares among this kernel, unfor_compare_range, unfor_select and unfor_aggregate, with the predicate
// arithmetic of fl_for_decide.hpp:
//   * a block's width, offset AND reference arrive together (three vector loads, one wait -- block_ref loads the reference
//     behind the data instead), its preconditions are checked (block_precondition: a failing block is skipped and its mask
//     words are left untouched, as unpack_widths leaves its output), then the block is decided;
//   * a DECIDED block (its fields' cyclic range lies inside, or outside, the predicate's interval) issues no packed load and
//     writes its 128-byte mask as all ones or all zeros;
//   * an undecided block fills its LDS image as unpack_widths does, and lane (i, c) funnels its cell of each 1-KiB group --
//     16/sizeof(T) consecutive indices -- adds c and compares with s (SWAR for u8 / u16, v_cmp for u32 / u64: row_predicate_bits
//     with W = T); the verdict bits are gathered into the first 128 bytes of the (by then dead) image and leave as ONE coalesced
//     128-byte store (lanes 0..7, 16 bytes each).
// LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_for_block.hpp"
#include "fl_for_decide.hpp"

namespace fl {

// WidthsArgs::refs and ::unpacked stay nullptr: the reference is loaded with the block's metadata, the output is the mask
struct ForCompareArgs : WidthsArgs {
    char* mask;                // [n_blocks][128 bytes]
    const void* cmp_refs;      // references[b * ref_stride]
    uint64_t cmp_a, cmp_s;     // the predicate: (v - cmp_a) mod 2^T <= cmp_s  (fl_for_decide.hpp, reduced on the host)
    unsigned cmp_none;         // 1: no value satisfies it
};

__device__ __forceinline__ ForPredicate predicate_of(const ForCompareArgs& a) { return ForPredicate{a.cmp_a, a.cmp_s, a.cmp_none != 0u}; }

// block `blk`'s 128-byte mask: lanes 0..7 store 16 bytes each, the descriptor drops the other lanes' stores
__device__ __forceinline__ void store_block_mask(const ForCompareArgs& a, uint64_t blk, u32x4 v, unsigned lane)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.mask + blk * 128u, 0, 128u, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, lane * 16u, 0, STORE_AUX);
}
__device__ __forceinline__ void store_decided_mask(const ForCompareArgs& a, uint64_t blk, int verdict, unsigned lane)
{
    const uint32_t m = verdict == FOR_CMP_ALL ? ~0u : 0u;
    store_block_mask(a, blk, u32x4{m, m, m, m}, lane);
}

// The LDS image of an undecided block (1 <= w <= T rows) -> its verdicts: bit e of verdicts[k] = element e of the lane's cell of group k
template <typename T>
__device__ __forceinline__ void compare_image_verdicts(const ForCompareArgs& a, unsigned w, const char* lds, unsigned lane, T c,
                                                       uint32_t (&verdicts)[WaveBlock<T>::GROUPS])
{
    constexpr int TB = WaveBlock<T>::TB;
    const Cell<T> cc = Cell<T>::splat(c);
    const T s = (T)a.cmp_s;
    for_each_funnelled_cell<T>(w, lds, lane, [&](auto K, unsigned bit, const Cell<T>& cell) {
        // ((f + c) mod 2^T) <= s per element: bit e = element e of the cell
        verdicts[decltype(K)::value] = row_predicate_bits<T, TB, false>(cell.add(cc), s);
    });
}

// The LDS image of an undecided block -> its mask: walk, gather (verdicts_to_image: the first 128 bytes of the by then dead image),
// and ONE coalesced 128-byte store
template <typename T>
__device__ __forceinline__ void compare_lds_image(const ForCompareArgs& a, uint64_t blk, unsigned w, char* lds, unsigned lane, T c)
{
    uint32_t verdicts[WaveBlock<T>::GROUPS];
    compare_image_verdicts<T>(a, w, lds, lane, c, verdicts);
    verdicts_to_image<T>(verdicts, lds, lane);
    store_block_mask(a, blk, *reinterpret_cast<const u32x4*>(lds + lane * 16u), lane);
}

// one block per call: metadata + reference, checks, verdict, and only for an undecided block the packed rows
template <typename T>
__device__ __forceinline__ void compare_block_wave(const ForCompareArgs& a, uint64_t blk, char* lds, unsigned lane)
{
    const BlockMeta m = settle_block_loads<T>(a, blk, issue_block_loads<T>(a, a.cmp_refs, blk));
    if (m.err) {
        raise_device_error(a.err_flag, m.err, lane);
        return;
    }
    uint64_t c;
    const int verdict = for_compare_decide(WaveBlock<T>::TB, predicate_of(a), m.r, m.w, c);
    if (verdict != FOR_CMP_EACH) {                                          // (W = 0 always ends here)
        store_decided_mask(a, blk, verdict, lane);
        return;
    }
    fill_block_image<T>(a, blk, m.off, m.w, lds, lane);
    compare_lds_image<T>(a, blk, m.w, lds, lane, (T)c);
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

// Several consecutive blocks per wavefront (the narrow types), as unpack_blocks_wave_prefetched: lane j judges block first + j --
// metadata, reference, preconditions and verdict -- BEFORE any packed load is issued; only the undecided blocks' rows are then
// requested by LDS-DMA, one image per block, one wait, and the blocks are answered back to back.
template <typename T>
__device__ __forceinline__ void compare_blocks_wave_prefetched(const ForCompareArgs& a, uint64_t first, unsigned count, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    const LaneBlocks<T> l = lane_block_loads<T>(a, a.cmp_refs, first, count, lane);
    uint64_t cv = 0;
    const int vv = l.ev ? (int)FOR_CMP_EACH : for_compare_decide(G::TB, predicate_of(a), l.rv, l.wv, cv);
    request_block_images<T>(a, l, __builtin_amdgcn_ballot_w64(l.owner && l.ev == 0u && vv == FOR_CMP_EACH), count, lds, lane);
    for (unsigned j = 0; j < count; ++j) {                    // wave-uniform loop
        const uint64_t blk = first + j;
        if (const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)l.ev, (int)j)) {
            raise_device_error(a.err_flag, e, lane);
            continue;
        }
        const int verdict = __builtin_amdgcn_readlane(vv, (int)j);
        if (verdict != FOR_CMP_EACH) {
            store_decided_mask(a, blk, verdict, lane);
            continue;
        }
        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)l.wv, (int)j);
        compare_lds_image<T>(a, blk, w, lds + j * G::BLOCK_BYTES, lane, (T)readlane_u64(cv, j));
    }
}

template <typename T>
__global__ __launch_bounds__(WG) void k_unfor_compare(ForCompareArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        if (a.prefetch && count > 1) {
            compare_blocks_wave_prefetched<T>(a, first, count, lds, lane);
            return;
        }
        for (unsigned j = 0; j < count; ++j) compare_block_wave<T>(a, first + j, lds, lane);
    });
}

typedef hipError_t (*for_compare_launch_t)(const ForCompareArgs&, int waves, hipStream_t);   // launch_block_consumer (fl_for_block.hpp)
template <typename T> for_compare_launch_t for_compare_launcher();

}  // namespace fl
