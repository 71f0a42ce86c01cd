// fl_aggregate.hpp -- unfor_aggregate: COUNT / SUM / MIN / MAX per block of a FoR-packed column, uniform or mixed width, over the rows a
// selection mask keeps (no mask: every row).
// EXTENSION (SURVEY.md 8 f2 "unpack -> filter" followed by a reduction), defined as a composition of reference functions:
//     V_b   = [ unfor_pack::<W_b>(block b, references[b * ref_stride])[i]  for i if bit i of block b ]
//     agg_b = { |V_b|, sum V_b (zero-extended to u64, wrapping), min V_b, max V_b }        (nothing kept: {0, 0, UINT64_MAX, 0})
// (ffor.rs:38-50; the mask in unpack_compare's layout).  It reads 128*W packed bytes and 128 mask bytes per block and writes 32.
// The wave-per-block machinery of fl_widths.hpp, through the steps fl_for_block.hpp shares among the four consumers of a packed column
// (the masks' stash is fl_select.hpp's):
//   * a block's width, offset, reference AND the lane's mask slices arrive together (independent vector loads, one wait); its
//     preconditions are checked (block_precondition): a failing block raises its bit and its slot receives the IDENTITY -- the slot feeds
//     a reduction (fl_scan.hpp: launch_aggregate_reduce), so a skipped block must not leave stale memory in it;
//   * a block whose mask is EMPTY, or whose width is 0, issues no packed load (fl_aggregate_map.hpp: aggregate_route);
//   * any other block fills its LDS image as unpack_widths does; lane l funnels its cell of each 1-KiB group, adds the reference and
//     accumulates, in registers, the elements whose slice bit is set (16 per lane for every type: 32-bit accumulators are exact for
//     u8 / u16, u32 / u64 take 64 bits);
//   * ONE butterfly over the 64 lanes (__shfl_xor) reduces count, sum, min and max together; the count is the popcount of the lane's mask
//     bits, never taken from the data path;
//   * lanes 0 and 1 store the slot's two 16-byte halves through a descriptor of exactly 32 bytes.
// LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_for_compare.hpp"
#include "fl_aggregate_map.hpp"
#include "fl_block_run.hpp"

namespace fl {

// WidthsArgs::refs and ::unpacked stay nullptr: the reference is loaded with the block's metadata, the output is one slot per block
struct AggregateArgs : WidthsArgs {
    const uint32_t* mask;          // [n_blocks][32]; nullptr = every row is kept (no mask is read)
    char* aggs;                    // [n_blocks] BlockAggregate
    const void* agg_refs;          // references[b * ref_stride]
};

// what a lane holds of its 16 elements: a block of u8 / u16 sums to less than 2^26
template <typename T> struct AggregateLane {
    using acc_t = std::conditional_t<sizeof(T) <= 2, uint32_t, uint64_t>;
    uint32_t count;
    acc_t sum, min, max;
};

// the lane's mask bits counted; nothing accumulated yet
template <typename T> __device__ __forceinline__ AggregateLane<T> aggregate_lane_of(const uint32_t (&slice)[SelectMap<sizeof(T)>::GROUPS])
{
    using acc_t = typename AggregateLane<T>::acc_t;
    AggregateLane<T> l{0u, (acc_t)0, ~(acc_t)0, (acc_t)0};
    static_for<(int)SelectMap<sizeof(T)>::GROUPS>([&](auto K) { l.count += (unsigned)__builtin_popcount(slice[decltype(K)::value]); });
    return l;
}

// the 64 lanes' partial aggregates -> the block's, in every lane: one butterfly, the four chains independent of each other
template <typename T> __device__ __forceinline__ BlockAggregate aggregate_wave_reduce(AggregateLane<T> l)
{
    using acc_t = typename AggregateLane<T>::acc_t;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t c = __shfl_xor(l.count, d, 64);
        const acc_t s = __shfl_xor(l.sum, d, 64), lo = __shfl_xor(l.min, d, 64), hi = __shfl_xor(l.max, d, 64);
        l.count += c;
        l.sum += s;
        l.min = lo < l.min ? lo : l.min;
        l.max = hi > l.max ? hi : l.max;
    }
    // only reached with count > 0: the narrow types' 32-bit minimum is then a value, not the accumulator's all-ones start
    return BlockAggregate{l.count, l.sum, l.min, l.max};
}

// the block's kept rows counted from the lanes' mask bits alone (the width-0 route)
__device__ __forceinline__ unsigned aggregate_wave_count(uint32_t c)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) c += __shfl_xor(c, d, 64);
    return (unsigned)__builtin_amdgcn_readfirstlane(c);
}

// block `blk`'s 32-byte slot (`g` wave-uniform): lane 0 stores {count, sum}, lane 1 {min, max}, the descriptor drops the other lanes
__device__ __forceinline__ void store_block_aggregate(const AggregateArgs& a, uint64_t blk, const BlockAggregate& g, unsigned lane)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.aggs + blk * sizeof(BlockAggregate), 0, (unsigned)sizeof(BlockAggregate), 0x00020000);
    const uint64_t x = lane == 0u ? g.count : g.min, y = lane == 0u ? g.sum : g.max;
    __builtin_amdgcn_raw_buffer_store_b128(u32x4{(uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32)}, rs, lane * 16u, 0, STORE_AUX);
}

// The LDS image of a block with 1 <= w <= T rows and a non-empty mask -> its aggregate (in every lane)
template <typename T>
__device__ __forceinline__ BlockAggregate aggregate_lds_image(unsigned w, const char* lds, unsigned lane, T ref, const uint32_t (&slice)[SelectMap<sizeof(T)>::GROUPS])
{
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    using acc_t = typename AggregateLane<T>::acc_t;
    static_assert(M::GROUPS == (unsigned)G::GROUPS && M::N == (unsigned)Elem<T>::PER_CELL, "fl_select_map.hpp follows fl_widths.hpp's lane map");
    const Cell<T> rc = Cell<T>::splat(ref);
    AggregateLane<T> l = aggregate_lane_of<T>(slice);
    for_each_funnelled_cell<T>(w, lds, lane, [&](auto K, unsigned bit, const Cell<T>& cell) {
        const Cell<T> v = cell.add(rc);                                     // ffor.rs:46-48
        const uint32_t sl = slice[decltype(K)::value];
        static_for<(int)M::N>([&](auto E) {
            constexpr unsigned e = decltype(E)::value;
            const acc_t x = (acc_t)cell_get<T>(v, (int)e);
            const bool on = ((sl >> e) & 1u) != 0u;
            l.sum += on ? x : (acc_t)0;
            l.min = on && x < l.min ? x : l.min;
            l.max = on && x > l.max ? x : l.max;
        });
    });
    return aggregate_wave_reduce<T>(l);
}

// one block per call: metadata, reference and the lane's mask slices in flight together
template <typename T>
__device__ __forceinline__ void aggregate_block_wave(const AggregateArgs& a, uint64_t blk, char* lds, unsigned lane)
{
    using M = SelectMap<sizeof(T)>;
    const BlockLoads<T> loads = issue_block_loads<T>(a, a.agg_refs, blk);
    uint32_t slice[M::GROUPS];
    block_mask_slices<T>(a.mask, blk, lane, slice);
    const BlockMeta m = settle_block_loads<T>(a, blk, loads);
    if (m.err) {
        raise_device_error(a.err_flag, m.err, lane);
        store_block_aggregate(a, blk, aggregate_identity(), lane);
        return;
    }
    uint32_t any = 0;
    static_for<(int)M::GROUPS>([&](auto K) { any |= slice[decltype(K)::value]; });
    const bool empty = __builtin_amdgcn_ballot_w64(any != 0u) == 0ull;
    const T r = (T)m.r;
    if (empty || m.w == 0u) {                                               // no packed load (fl_aggregate_map.hpp)
        const unsigned count = empty ? 0u : aggregate_wave_count(aggregate_lane_of<T>(slice).count);
        store_block_aggregate(a, blk, aggregate_constant_block(count, (uint64_t)r), lane);
        return;
    }
    fill_block_image<T>(a, blk, m.off, m.w, lds, lane);
    store_block_aggregate(a, blk, aggregate_lds_image<T>(m.w, lds, lane, r, slice), lane);
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

// BPW consecutive blocks per wavefront (the narrow types' shipped shapes: static_shape), as select_blocks_wave_static: lane j judges block
// first + j -- metadata, reference, preconditions -- and the wavefront reads the BPW masks into its stash, BEFORE any packed load is
// issued; only the rows of the blocks that need a decode are then requested by LDS-DMA, one image per block, one wait, and the blocks
// are aggregated back to back.
template <typename T, unsigned BPW>
__device__ __forceinline__ void aggregate_blocks_wave_static(const AggregateArgs& a, uint64_t first, char* lds, uint32_t* stash, unsigned lane)
{
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    const LaneBlocks<T> l = lane_block_loads<T>(a, a.agg_refs, first, BPW, lane);
    const unsigned nonempty = stash_block_masks<BPW>(a.mask, first, stash, lane);
    request_block_images<T, BPW>(a, l, __builtin_amdgcn_ballot_w64(l.owner && l.ev == 0u) & nonempty, lds, lane);
    for (unsigned j = 0; j < BPW; ++j) {                                    // wave-uniform loop
        const uint64_t blk = first + j;
        if (const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)l.ev, (int)j)) {
            raise_device_error(a.err_flag, e, lane);
            store_block_aggregate(a, blk, aggregate_identity(), lane);
            continue;
        }
        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)l.wv, (int)j);
        const T r = readlane_elem<T>(l.rv, j);
        uint32_t slice[M::GROUPS];
        stashed_slices<T>(stash, j, lane, slice);
        const bool empty = !((nonempty >> j) & 1u);
        if (empty || w == 0u) {                                             // nothing was fetched (fl_aggregate_map.hpp)
            const unsigned count = empty ? 0u : aggregate_wave_count(aggregate_lane_of<T>(slice).count);
            store_block_aggregate(a, blk, aggregate_constant_block(count, (uint64_t)r), lane);
            continue;
        }
        store_block_aggregate(a, blk, aggregate_lds_image<T>(w, lds + j * G::BLOCK_BYTES, lane, r, slice), lane);
    }
}

template <typename T>
__global__ __launch_bounds__(WG) void k_unfor_aggregate(AggregateArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        if constexpr (sizeof(T) <= 2) {                       // the shipped shapes of the narrow types; any other shape: block by block
            if (static_shape<T>(a.bpw, a.prefetch) && count == a.bpw) {
                uint32_t* stash = wave_mask_stash<T>(a.bpw);
                if (a.bpw == 4) aggregate_blocks_wave_static<T, 4>(a, first, lds, stash, lane);
                else aggregate_blocks_wave_static<T, 2>(a, first, lds, stash, lane);
                return;
            }
        }
        for (unsigned j = 0; j < count; ++j) aggregate_block_wave<T>(a, first + j, lds, lane);
    });
}

typedef hipError_t (*aggregate_launch_t)(const AggregateArgs&, int waves, hipStream_t);   // launch_block_consumer (fl_for_block.hpp), with the stash
template <typename T> aggregate_launch_t aggregate_launcher();

}  // namespace fl
