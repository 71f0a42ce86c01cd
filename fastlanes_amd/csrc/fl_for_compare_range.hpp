// fl_for_compare_range.hpp -- unfor_compare_range: an interval predicate over a FoR-packed column, uniform or mixed width, chained
// through the mask so far.  EXTENSION, defined as a composition of reference functions; all arithmetic mod 2^T:
//     hit[b][i] = ((unfor_pack::<W_b>(block b, references[b * ref_stride])[i] - lo) mod 2^T) <= ((hi - lo) mod 2^T)
//     NEW: mask[b] = hit[b]      AND: mask[b] = mask_in[b] & hit[b]      OR: mask[b] = mask_in[b] | hit[b]
// (ffor.rs:38-50; the masks in unpack_compare's layout, 32 words per block).  The cyclic interval [lo, hi] IS the ForPredicate the
// compare kernel already evaluates (fl_for_decide.hpp: for_range_predicate), so this is k_unfor_compare (fl_for_compare.hpp) with
// the incoming mask beside it:
//   * a block's 128 bytes of mask_in arrive with its width, offset and reference (independent vector loads, one wait); lanes 0..7
//     hold 16 bytes each -- the shape store_block_mask stores in;
//   * a block is answered WITHOUT a packed load when for_compare_decide decides it from reference and width, when the combiner is
//     AND and its incoming mask is all zero, or when the combiner is OR and its incoming mask is all ones (one ballot serves both);
//   * an undecided block gathers its verdict bits in the dead LDS image through compare_lds_image's own walk and gather
//     (compare_image_verdicts, verdicts_to_image), and they are combined with the lane's 16 bytes just before the one coalesced
//     128-byte store;
//   * a block that fails the mixed-width device checks is skipped: its FL_DEVERR_* bit is raised, its mask words are left alone.
// Every valid block's 128 bytes are always written.  `mask` may be `mask_in` itself: a wavefront has read the incoming masks of all
// the blocks it owns before it stores the first of them, and no other wavefront touches those bytes.
// LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_for_compare.hpp"

namespace fl {

enum MaskCombine { MASK_NEW = 0, MASK_AND = 1, MASK_OR = 2 };   // include/fastlanes_amd.h: fl_mask_combine

struct ForRangeArgs : ForCompareArgs {
    const char* mask_in;       // [n_blocks][128 bytes]; nullptr with MASK_NEW
    unsigned combine;          // MaskCombine
};

__device__ __forceinline__ u32x4 range_combine(unsigned combine, u32x4 in, u32x4 hit)
{
    return combine == MASK_AND ? (in & hit) : combine == MASK_OR ? (in | hit) : hit;
}

// true if this lane's 16 bytes leave the block's answer open: a set bit under AND, a clear bit under OR (NEW: always)
__device__ __forceinline__ bool range_mask_live(unsigned combine, u32x4 in)
{
    if (combine == MASK_AND) return (in[0] | in[1] | in[2] | in[3]) != 0u;
    if (combine == MASK_OR) return (in[0] & in[1] & in[2] & in[3]) != ~0u;
    return true;
}

// block `blk`'s 128-byte mask from lanes base .. base + 7, 16 bytes each; every other lane's store lands past the descriptor
__device__ __forceinline__ void store_range_mask(const ForRangeArgs& a, uint64_t blk, u32x4 v, unsigned lane, unsigned base)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.mask + blk * 128u, 0, 128u, 0x00020000);
    const unsigned rel = lane - base;
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, rel < 8u ? rel * 16u : 128u, 0, STORE_AUX);
}
__device__ __forceinline__ void store_decided_range(const ForRangeArgs& a, uint64_t blk, int verdict, u32x4 in, unsigned lane, unsigned base)
{
    const uint32_t m = verdict == FOR_CMP_ALL ? ~0u : 0u;
    store_range_mask(a, blk, range_combine(a.combine, in, u32x4{m, m, m, m}), lane, base);
}

// The LDS image of an undecided block -> its mask: compare_lds_image's walk and gather, then the verdict bits are combined with `in`
// = the 16 bytes lanes base .. base + 7 hold of block `blk`'s mask_in
template <typename T>
__device__ __forceinline__ void combine_lds_image(const ForRangeArgs& a, uint64_t blk, unsigned w, char* lds, unsigned lane, T c, u32x4 in, unsigned base)
{
    uint32_t verdicts[WaveBlock<T>::GROUPS];
    compare_image_verdicts<T>(a, w, lds, lane, c, verdicts);
    verdicts_to_image<T>(verdicts, lds, lane);
    // lane base + i reads the 16 bytes lane i of the compare kernel stores (base is a multiple of 8)
    store_range_mask(a, blk, range_combine(a.combine, in, *reinterpret_cast<const u32x4*>(lds + (lane & 7u) * 16u)), lane, base);
}

// one block per call: metadata, reference and the incoming mask in flight together; only an open block requests its packed rows
template <typename T>
__device__ __forceinline__ void range_block_wave(const ForRangeArgs& a, uint64_t blk, char* lds, unsigned lane)
{
    const BlockLoads<T> loads = issue_block_loads<T>(a, a.cmp_refs, blk);
    u32x4 in = {0u, 0u, 0u, 0u};
    if (a.combine != MASK_NEW) {
        // exactly this block's 128 bytes: lanes 8..63 read past the descriptor, which returns 0 and touches no memory
        const __amdgpu_buffer_rsrc_t ms = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.mask_in) + blk * 128u, 0, 128u, 0x00020000);
        in = __builtin_amdgcn_raw_buffer_load_b128(ms, lane * 16u, 0, 0);
    }
    const BlockMeta m = settle_block_loads<T>(a, blk, loads);
    if (m.err) {
        raise_device_error(a.err_flag, m.err, lane);
        return;
    }
    if (__builtin_amdgcn_ballot_w64(lane < 8u && range_mask_live(a.combine, in)) == 0ull) {
        store_range_mask(a, blk, in, lane, 0u);                             // AND of nothing, OR of everything: mask_in is the answer
        return;
    }
    uint64_t c;
    const int verdict = for_compare_decide(WaveBlock<T>::TB, predicate_of(a), m.r, m.w, c);
    if (verdict != FOR_CMP_EACH) {                                          // (W = 0 always ends here)
        store_decided_range(a, blk, verdict, in, lane, 0u);
        return;
    }
    fill_block_image<T>(a, blk, m.off, m.w, lds, lane);
    combine_lds_image<T>(a, blk, m.w, lds, lane, (T)c, in, 0u);
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

// Several consecutive blocks per wavefront (the narrow types), as compare_blocks_wave_prefetched: lane j judges block first + j --
// metadata, reference, preconditions, verdict -- and lanes 8j .. 8j + 7 hold its incoming mask (two loads cover 16 blocks), BEFORE
// any packed load is issued; only the blocks still open are then requested by LDS-DMA, one image per block, one wait, and the
// blocks are answered back to back, each stored by the eight lanes that hold its incoming bytes.
template <typename T>
__device__ __forceinline__ void range_blocks_wave_prefetched(const ForRangeArgs& a, uint64_t first, unsigned count, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    const LaneBlocks<T> l = lane_block_loads<T>(a, a.cmp_refs, first, count, lane);
    u32x4 in[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};      // in[h]: 16 bytes of block first + 8h + lane / 8
    uint64_t live[2] = {~0ull, ~0ull};
    if (a.combine != MASK_NEW) {
        // exactly the wavefront's count * 128 bytes: lanes past them read 0 and touch no memory
        const __amdgpu_buffer_rsrc_t ms = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.mask_in) + first * 128u, 0, count * 128u, 0x00020000);
        in[0] = __builtin_amdgcn_raw_buffer_load_b128(ms, lane * 16u, 0, 0);
        if (count > 8u) in[1] = __builtin_amdgcn_raw_buffer_load_b128(ms, lane * 16u + 1024u, 0, 0);
        live[0] = __builtin_amdgcn_ballot_w64(range_mask_live(a.combine, in[0]));
        live[1] = __builtin_amdgcn_ballot_w64(range_mask_live(a.combine, in[1]));
    }
    uint64_t cv = 0;
    const int vv = l.ev ? (int)FOR_CMP_EACH : for_compare_decide(G::TB, predicate_of(a), l.rv, l.wv, cv);
    // bit j: block first + j's answer is still open after its incoming mask (byte j % 8 of live[j / 8])
    unsigned open_blocks = 0;
    for (unsigned j = 0; j < count; ++j)                      // wave-uniform
        open_blocks |= (((live[j >> 3] >> (8u * (j & 7u))) & 0xffull) != 0ull ? 1u : 0u) << j;
    request_block_images<T>(a, l, __builtin_amdgcn_ballot_w64(l.owner && l.ev == 0u && vv == FOR_CMP_EACH) & open_blocks, count, lds, lane);
    for (unsigned j = 0; j < count; ++j) {                    // wave-uniform loop
        const uint64_t blk = first + j;
        if (const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)l.ev, (int)j)) {
            raise_device_error(a.err_flag, e, lane);
            continue;
        }
        const u32x4 mi = j < 8u ? in[0] : in[1];
        const unsigned base = 8u * (j & 7u);
        if (!((open_blocks >> j) & 1u)) {
            store_range_mask(a, blk, mi, lane, base);          // AND of nothing, OR of everything: mask_in is the answer
            continue;
        }
        const int verdict = __builtin_amdgcn_readlane(vv, (int)j);
        if (verdict != FOR_CMP_EACH) {
            store_decided_range(a, blk, verdict, mi, lane, base);
            continue;
        }
        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)l.wv, (int)j);
        combine_lds_image<T>(a, blk, w, lds + j * G::BLOCK_BYTES, lane, (T)readlane_u64(cv, j), mi, base);
    }
}

template <typename T>
__global__ __launch_bounds__(WG) void k_unfor_compare_range(ForRangeArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        if (a.prefetch && count > 1) {
            range_blocks_wave_prefetched<T>(a, first, count, lds, lane);
            return;
        }
        for (unsigned j = 0; j < count; ++j) range_block_wave<T>(a, first + j, lds, lane);
    });
}

typedef hipError_t (*for_range_launch_t)(const ForRangeArgs&, int waves, hipStream_t);   // launch_block_consumer (fl_for_block.hpp)
template <typename T> for_range_launch_t for_range_launcher();

}  // namespace fl
