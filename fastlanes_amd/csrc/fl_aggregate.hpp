// fl_aggregate.hpp -- unfor_aggregate: COUNT / SUM / MIN / MAX per block of a FoR-packed column, uniform or mixed width, over the rows a
// selection mask keeps (no mask: every row).
// EXTENSION (SURVEY.md 8 f2 "unpack -> filter" followed by a reduction), defined as a composition of reference functions:
//     V_b   = [ unfor_pack::<W_b>(block b, references[b * ref_stride])[i]  for i if bit i of block b ]
//     agg_b = { |V_b|, sum V_b (zero-extended to u64, wrapping), min V_b, max V_b }        (nothing kept: {0, 0, UINT64_MAX, 0})
// (ffor.rs:38-50; the mask in unpack_compare's layout).  It reads 128*W packed bytes and 128 mask bytes per block and writes 32.
// The wave-per-block machinery of fl_widths.hpp, as in fl_select.hpp:
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
#include "fl_widths.hpp"
#include "fl_for_compare.hpp"
#include "fl_select_map.hpp"
#include "fl_aggregate_map.hpp"

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
    constexpr int TB = G::TB;
    static_assert(M::GROUPS == (unsigned)G::GROUPS && M::N == (unsigned)Elem<T>::PER_CELL, "fl_select_map.hpp follows fl_widths.hpp's lane map");
    const unsigned c16 = (lane & 7u) * 16u;
    const typename G::word_t m = G::field_mask(w);
    unsigned bit = __umul24(G::row_base(lane >> 3), w);
    const unsigned step = G::KSTEP * w;
    const unsigned last = (w - 1u) * 128u;
    const Cell<T> rc = Cell<T>::splat(ref);
    AggregateLane<T> l = aggregate_lane_of<T>(slice);
    static_for<G::GROUPS>([&](auto K) {
        const unsigned word = bit >> G::LOG_TB, sh = bit & (TB - 1u);
        const unsigned a0 = word * 128u;
        const unsigned a1 = a0 + 128u < last ? a0 + 128u : last;            // the last row never reads past the end (macros.rs:156)
        const Cell<T> cur = __builtin_bit_cast(Cell<T>, *reinterpret_cast<const u32x4*>(lds + a0 + c16));
        const Cell<T> nxt = __builtin_bit_cast(Cell<T>, *reinterpret_cast<const u32x4*>(lds + a1 + c16));
        const Cell<T> v = G::funnel(cur, nxt, sh, m).add(rc);               // ffor.rs:46-48
        const uint32_t sl = slice[decltype(K)::value];
        static_for<(int)M::N>([&](auto E) {
            constexpr unsigned e = decltype(E)::value;
            const acc_t x = (acc_t)cell_get<T>(v, (int)e);
            const bool on = ((sl >> e) & 1u) != 0u;
            l.sum += on ? x : (acc_t)0;
            l.min = on && x < l.min ? x : l.min;
            l.max = on && x > l.max ? x : l.max;
        });
        bit += step;
    });
    return aggregate_wave_reduce<T>(l);
}

// one block per call: metadata, reference and the lane's mask slices in flight together
template <typename T>
__device__ __forceinline__ void aggregate_block_wave(const AggregateArgs& a, uint64_t blk, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    constexpr int TB = G::TB;
    const unsigned z = opaque_zero();
    unsigned wv = a.uniform_width;
    uint64_t ov = 0;
    if (a.widths) wv = a.widths[blk + z];
    if (a.offsets) ov = a.offsets[blk + z];
    const T rv = static_cast<const T*>(a.agg_refs)[blk * a.ref_stride + z];
    uint32_t slice[M::GROUPS];
    static_for<(int)M::GROUPS>([&](auto K) {
        constexpr unsigned k = decltype(K)::value;
        slice[k] = (1u << M::N) - 1u;                                       // no mask: every row
        if (a.mask) slice[k] = M::slice(a.mask[blk * SELECT_MASK_WORDS + M::mask_word(k, lane)], k, lane);
    });
    const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(wv);
    const uint64_t off = a.offsets ? wave_uniform_u64(ov) : blk * (uint64_t)(128u * w);
    const T r = (T)wave_uniform_u64((uint64_t)rv);
    if (const uint32_t e = block_precondition(a, w, off, TB)) {            // bitpacking.rs:126 unreachable!(), :111-113
        raise_device_error(a.err_flag, e, lane);
        store_block_aggregate(a, blk, aggregate_identity(), lane);
        return;
    }
    uint32_t any = 0;
    static_for<(int)M::GROUPS>([&](auto K) { any |= slice[decltype(K)::value]; });
    const bool empty = __builtin_amdgcn_ballot_w64(any != 0u) == 0ull;
    if (empty || w == 0u) {                                                 // no packed load (fl_aggregate_map.hpp)
        const unsigned count = empty ? 0u : aggregate_wave_count(aggregate_lane_of<T>(slice).count);
        store_block_aggregate(a, blk, aggregate_constant_block(count, (uint64_t)r), lane);
        return;
    }
    // wave-uniform descriptor over exactly this block's 128*w bytes: cells past it read as 0, no fault
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.packed) + off, 0, 128u * w, 0x00020000);
    Cell<T> no_ref;
    if (a.widths || w >= a.nt_from) packed_block_to_lds<T, RD_DMA_NT>(a, blk, rs, w, lds, lane, no_ref);   // RD_AUTO (fl_widths.hpp)
    else packed_block_to_lds<T, RD_VGPR>(a, blk, rs, w, lds, lane, no_ref);
    wave_lds_fence();
    store_block_aggregate(a, blk, aggregate_lds_image<T>(w, lds, lane, r, slice), lane);
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

// the launch shapes aggregate_blocks_wave_static serves (any other shape runs block by block through the wavefront's first image)
template <typename T> __host__ __device__ inline bool aggregate_static_shape(unsigned bpw, unsigned prefetch)
{
    return sizeof(T) <= 2 && prefetch != 0u && (bpw == 2u || bpw == 4u);
}

// BPW consecutive blocks per wavefront (the narrow types' shipped shapes), as select_blocks_wave_static: lane j judges block first + j --
// metadata, reference, preconditions -- and the wavefront reads the BPW masks (two blocks per load) into `stash`, BEFORE any packed load
// is issued; only the rows of the blocks that need a decode are then requested by LDS-DMA, one image per block, one wait, and the blocks
// are aggregated back to back.  `stash`: BPW * 128 bytes of wave-private LDS behind the images.
template <typename T, unsigned BPW>
__device__ __forceinline__ void aggregate_blocks_wave_static(const AggregateArgs& a, uint64_t first, char* lds, uint32_t* stash, unsigned lane)
{
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    constexpr int TB = G::TB;
    static_assert(BPW >= 2 && BPW <= 16 && BPW % 2 == 0, "two blocks' masks per load");
    const bool owner = lane < BPW;
    const uint64_t mine = first + (owner ? lane : 0u);
    unsigned wv = a.uniform_width;
    if (a.widths) wv = a.widths[mine];
    uint64_t ov = mine * (uint64_t)(128u * wv);
    if (a.offsets) ov = a.offsets[mine];
    const T rv = static_cast<const T*>(a.agg_refs)[mine * a.ref_stride];
    uint32_t mw[BPW / 2];
    static_for<(int)(BPW / 2)>([&](auto I) {
        constexpr unsigned i = decltype(I)::value;
        mw[i] = ~0u;                                                        // no mask: every row
        if (a.mask) mw[i] = a.mask[(first + 2u * i) * SELECT_MASK_WORDS + lane];   // words of blocks first + 2i (lanes 0..31) and first + 2i + 1
    });
    const uint32_t ev = block_precondition(a, wv, ov, TB);
    unsigned nonempty = 0;                                                  // wave-uniform: bit j = block first + j keeps something
    static_for<(int)(BPW / 2)>([&](auto I) {
        constexpr unsigned i = decltype(I)::value;
        stash[i * 64u + lane] = mw[i];
        const uint64_t nz = __builtin_amdgcn_ballot_w64(mw[i] != 0u);
        nonempty |= ((uint32_t)nz != 0u ? 1u : 0u) << (2u * i) | ((uint32_t)(nz >> 32) != 0u ? 2u : 0u) << (2u * i);
    });
    const uint64_t valid = __builtin_amdgcn_ballot_w64(owner && ev == 0u);
    const uint64_t fetch = valid & nonempty;                                // (a width-0 block requests nothing: 8 * g < 0 never holds)
    static_for<(int)BPW>([&](auto J) {
        constexpr unsigned j = decltype(J)::value;
        if ((fetch >> j) & 1u) {
            const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)wv, (int)j);
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.packed) + readlane_u64(ov, j), 0, 128u * w, 0x00020000);
            char* img = lds + j * G::BLOCK_BYTES;
            static_for<G::GROUPS>([&](auto Gi) {
                constexpr int g = decltype(Gi)::value;
                if (8u * g < w) dma_1k_to_lds<RD_DMA_NT, g * 1024>(rs, img, lane);
            });
        }
    });
    wait_lds_dma();
    wave_lds_fence();
    for (unsigned j = 0; j < BPW; ++j) {                                    // wave-uniform loop
        const uint64_t blk = first + j;
        if (const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)ev, (int)j)) {   // bitpacking.rs:126 unreachable!(), :111-113
            raise_device_error(a.err_flag, e, lane);
            store_block_aggregate(a, blk, aggregate_identity(), lane);
            continue;
        }
        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)wv, (int)j);
        const T r = readlane_elem<T>(rv, j);
        uint32_t slice[M::GROUPS];
        static_for<(int)M::GROUPS>([&](auto K) {
            constexpr unsigned k = decltype(K)::value;
            slice[k] = M::slice(stash[j * SELECT_MASK_WORDS + M::mask_word(k, lane)], k, lane);
        });
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
            if (aggregate_static_shape<T>(a.bpw, a.prefetch) && count == a.bpw) {
                extern __shared__ __attribute__((aligned(16))) char lds_all[];
                const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
                uint32_t* stash = reinterpret_cast<uint32_t*>(lds_all + (WG / 64) * WaveBlock<T>::BLOCK_BYTES * a.bpw) + wave * a.bpw * SELECT_MASK_WORDS;
                if (a.bpw == 4) aggregate_blocks_wave_static<T, 4>(a, first, lds, stash, lane);
                else aggregate_blocks_wave_static<T, 2>(a, first, lds, stash, lane);
                return;
            }
        }
        for (unsigned j = 0; j < count; ++j) aggregate_block_wave<T>(a, first + j, lds, lane);
    });
}

// Launched with the shape of unfor_pack_widths (the C ABI passes fl_dispatch.hpp's mixed_* choices through with_policy); the tile map is
// plan_blocks', rotated for mixed-width columns as in launch_widths.  The masks' stash rides behind the workgroup's block images.
typedef hipError_t (*aggregate_launch_t)(const AggregateArgs&, int waves, hipStream_t);
template <typename T> hipError_t launch_unfor_aggregate(const AggregateArgs& a0, int waves, hipStream_t s)
{
    if (a0.n_blocks == 0) return hipSuccess;
    AggregateArgs a = a0;
    const unsigned need = tidy_wave_blocks<T>(a.bpw, a.prefetch) + (aggregate_static_shape<T>(a.bpw, a.prefetch) ? (WG / 64) * a.bpw * SELECT_MASK_WORDS * 4u : 0u);
    const unsigned grid = plan_blocks(a, a.n_blocks, a.bpw * (WG / 64), WIN_UNPACK, WaveBlock<T>::TB, a.widths != nullptr);
    const unsigned lds = occupancy_lds(waves, need);
    if (!grid || lds > 64 * 1024) return hipErrorInvalidValue;         // > 2^33 blocks; beyond the default dynamic-LDS limit
    FL_LAUNCH((k_unfor_aggregate<T>), dim3(grid), dim3(WG), lds, s, a);
    return hipGetLastError();
}
template <typename T> aggregate_launch_t aggregate_launcher();

}  // namespace fl
