// fl_delta_aggregate.hpp -- undelta_aggregate: COUNT / SUM / MIN / MAX per block of a DELTA-packed column, uniform or mixed width, over the
// rows a selection mask keeps (no mask: every row).  EXTENSION, defined as a composition of reference functions;
// arithmetic mod 2^T unless stated:
//     v[b]  = untranspose(undelta_pack::<W_b>(block b, bases[b * LANES .. + LANES]))             (delta.rs:47-63, transpose.rs:17-22)
//     V_b   = [ v[b][i]  for i if bit i of block b of mask ]          mask == NULL: every i, and no mask is read
//     agg_b = { count = |V_b|, sum = sum of V_b zero-extended to u64 (wrapping mod 2^64), min = min V_b, max = max V_b }
//             nothing kept: the identity {0, 0, UINT64_MAX, 0}
// The mask is the one every compare entry point writes and undelta_compare_range produces: 32 words per block, bit i = ORIGINAL row i,
// LSB first.  The slot is fl_block_aggregate; slots, identity, determinism and the reduction (fl_aggregate_reduce) are unfor_aggregate's
// (fl_aggregate.hpp).
// It rests on the lane-group fact of fl_delta_compare_range_map.hpp: the T chained rows of FastLanes lane l are the T consecutive
// original rows lane_base(l) .. + T - 1, so the mask bits that govern one chain are the aligned T-bit group at bit delta_group_bit(l);
// add, min and max do not care about order, so the chains are aggregated where they are decoded and no value is untransposed.
// One wavefront per block, launched through the block-consumer plan as k_undelta_compare_range is:
//   * the block's width, offset, its 128 bytes of bases and its 128 bytes of mask are independent vector loads under one wait; lane
//     (i, c) holds the bases of cell column c (FL lanes N c .. N c + N - 1, N = 16 / sizeof(T));
//   * the route is fl_delta_aggregate_map.hpp's: SKIP (a device check failed: the bit is raised, the slot receives the identity),
//     IDENTITY (an empty mask), BASES (W = 0) -- none of them requests a packed byte -- and EACH;
//   * the lane's mask bits: lanes 0..7 lay the mask's 128 bytes into the still unused LDS image and every lane reads the N groups of its
//     cell column into groups_of_rows' layout (group e at bits e T .. of v[0..3]) -- the inverse of place_groups -- then a fence, and only
//     then is the image filled (u64: a lane's two groups ARE 16 bytes of the mask, which every lane loads itself; nothing is staged).
//     Without a mask nothing is loaded or staged;
//   * EACH fills the LDS image and takes the lane's R = T/8 consecutive rows through fl_chain.hpp's stages as they are
//     (chain_stage_source<SRC_PACKED, CHAIN_NONE>, chain_stage_rows<SRC_PACKED, CHAIN_UNDELTA>) with the plain bases: lane (i, c) holds
//     rows R i .. R i + R - 1 of its N chains, 16 elements for every type (AggregateLane<T>'s 32-bit accumulators are exact for u8 /
//     u16); element e of row j is accumulated under bit R i + j of group e; the count is the popcount of the lane's own R-bit pieces,
//     never taken from the data path, and each mask bit is counted by exactly one lane; then aggregate_wave_reduce and
//     store_block_aggregate, unchanged;
//   * BASES uses the same registers: lanes 0..7 hold every group whole, and add their N chains (delta_aggregate_add_chain).
// LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_aggregate.hpp"
#include "fl_delta_compare_range.hpp"
#include "fl_delta_aggregate_map.hpp"

namespace fl {

// AggregateArgs::agg_refs and ::ref_stride are unused: a Delta block has LANES bases, not one reference
struct DeltaAggregateArgs : AggregateArgs {
    const char* bases;         // [n_blocks][128 bytes]
};

// The N whole mask groups of the lane's cell column (FL lanes N c + e), group e at bits e T .. e T + T - 1 of v[0..3], in EVERY lane.
// u64: `in` is bytes 16 c .. 16 c + 15 of the block's mask, which are the two groups.  Narrower: lanes 0..7 hold the mask's 128 bytes
// (`in` = bytes 16 lane ..), and the groups are gathered through the first 128 bytes of the wavefront's LDS image, which must be unused.
template <typename T> __device__ __forceinline__ void lane_mask_groups(const u32x4& in, char* lds, unsigned lane, uint32_t (&v)[4])
{
    constexpr int TB = WaveBlock<T>::TB, N = Elem<T>::PER_CELL;
    if constexpr (TB == 64) {
        for (int k = 0; k < 4; ++k) v[k] = in[k];
    } else {
        if (lane < 8u) *reinterpret_cast<u32x4*>(lds + lane * 16u) = in;
        wave_lds_fence();
        for (int k = 0; k < 4; ++k) v[k] = 0u;
        static_for<N>([&](auto E) {
            constexpr int e = decltype(E)::value;
            const char* at = lds + delta_group_bit((unsigned)N * (lane & 7u) + e) / 8u;
            if constexpr (TB == 32) v[e] = *reinterpret_cast<const uint32_t*>(at);
            else if constexpr (TB == 16) v[e >> 1] |= (uint32_t)*reinterpret_cast<const uint16_t*>(at) << (16 * (e & 1));
            else v[e >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(at) << (8 * (e & 3));
        });
        wave_lds_fence();                                                       // every lane holds its groups: the image may be filled
    }
}
// the lane's own pieces, rows R i .. R i + R - 1 of each group: bit e R + j <-> element e of the lane's row R i + j (16 bits)
template <typename T> __device__ __forceinline__ uint32_t lane_piece_bits(const uint32_t (&v)[4], unsigned i)
{
    constexpr int TB = WaveBlock<T>::TB, R = TB / 8, N = Elem<T>::PER_CELL;
    uint32_t bits = 0u;
    static_for<N>([&](auto E) {
        constexpr int e = decltype(E)::value;
        if constexpr (TB == 64) {
            const uint64_t g = (((uint64_t)v[2 * e + 1] << 32) | v[2 * e]) >> (8u * i);
            bits |= ((uint32_t)g & 0xffu) << (8 * e);
        } else {
            bits |= ((v[(e * TB) >> 5] >> (((e * TB) & 31) + (unsigned)R * i)) & ((1u << R) - 1u)) << (R * e);
        }
    });
    return bits;
}
// the kept rows of whole group e
template <typename T> __device__ __forceinline__ unsigned group_popcount(const uint32_t (&v)[4], int e)
{
    constexpr int TB = WaveBlock<T>::TB;
    if constexpr (TB == 64) return (unsigned)(__builtin_popcount(v[2 * e]) + __builtin_popcount(v[2 * e + 1]));
    else if constexpr (TB == 32) return (unsigned)__builtin_popcount(v[e]);
    else return (unsigned)__builtin_popcount((v[(e * TB) >> 5] >> ((e * TB) & 31)) & ((1u << TB) - 1u));
}

// one block per call
template <typename T>
__device__ __forceinline__ void delta_aggregate_block_wave(const DeltaAggregateArgs& a, uint64_t blk, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    using acc_t = typename AggregateLane<T>::acc_t;
    constexpr int TB = G::TB, R = TB / 8, N = Elem<T>::PER_CELL;
    // width, offset, bases and the mask: independent vector loads, one wait
    const unsigned z = opaque_zero();
    unsigned wv = a.uniform_width;
    uint64_t ov = 0;
    if (a.widths) wv = a.widths[blk + z];
    if (a.offsets) ov = a.offsets[blk + z];
    const Cell<T> base = __builtin_bit_cast(Cell<T>, *reinterpret_cast<const u32x4*>(a.bases + blk * 128u + (lane & 7u) * 16u + z));
    u32x4 in = {~0u, ~0u, ~0u, ~0u};
    if (a.mask) {
        // exactly this block's 128 bytes: a lane that reads past the descriptor receives 0 and touches no memory
        const __amdgpu_buffer_rsrc_t ms = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(a.mask) + blk * 32u, 0, 128u, 0x00020000);
        in = __builtin_amdgcn_raw_buffer_load_b128(ms, (TB == 64 ? (lane & 7u) : lane) * 16u, 0, 0);
    }
    const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(wv);
    const uint64_t off = a.offsets ? wave_uniform_u64(ov) : blk * (uint64_t)(128u * w);
    if (const uint32_t e = block_precondition(a, w, off, TB)) {                 // SKIP
        raise_device_error(a.err_flag, e, lane);
        store_block_aggregate(a, blk, aggregate_identity(), lane);
        return;
    }
    if (a.mask && __builtin_amdgcn_ballot_w64(lane < 8u && (in[0] | in[1] | in[2] | in[3]) != 0u) == 0ull) {
        store_block_aggregate(a, blk, aggregate_identity(), lane);              // IDENTITY
        return;
    }
    uint32_t v[4] = {~0u, ~0u, ~0u, ~0u};
    if (a.mask) lane_mask_groups<T>(in, lds, lane, v);
    if (w == 0u) {                                                              // BASES: each chain repeats its base
        BlockAggregate g = aggregate_identity();
        static_for<N>([&](auto E) {
            constexpr int e = decltype(E)::value;
            delta_aggregate_add_chain(g, lane < 8u ? group_popcount<T>(v, e) : 0u, cell_get<T>(base, e));
        });
        store_block_aggregate(a, blk, aggregate_wave_reduce<uint64_t>(AggregateLane<uint64_t>{(uint32_t)g.count, g.sum, g.min, g.max}), lane);
        if constexpr (TB != 64) wave_lds_fence();                               // the staged mask is overwritten by the wavefront's next block
        return;
    }
    const ChainArgs ca = chain_source_args(a);
    Cell<T> unused;
    chain_stage_source<T, SRC_PACKED, CHAIN_NONE, RD_AUTO>(ca, blk, w, off, lds, lane, unused);
    wave_lds_fence();
    Cell<T> x[R];
    chain_stage_rows<T, SRC_PACKED, CHAIN_UNDELTA>(w, lds, lane, base, x);
    const uint32_t bits = lane_piece_bits<T>(v, lane >> 3);
    AggregateLane<T> l{(uint32_t)__builtin_popcount(bits), (acc_t)0, ~(acc_t)0, (acc_t)0};
    static_for<R>([&](auto J) {
        static_for<N>([&](auto E) {
            constexpr int j = decltype(J)::value, e = decltype(E)::value;
            const acc_t y = (acc_t)cell_get<T>(x[j], e);
            const bool on = ((bits >> (e * R + j)) & 1u) != 0u;
            l.sum += on ? y : (acc_t)0;
            l.min = on && y < l.min ? y : l.min;
            l.max = on && y > l.max ? y : l.max;
        });
    });
    store_block_aggregate(a, blk, aggregate_wave_reduce<T>(l), lane);
    wave_lds_fence();                                                           // the image is reused by the wavefront's next block
}

template <typename T>
__global__ __launch_bounds__(WG) void k_undelta_aggregate(DeltaAggregateArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        for (unsigned j = 0; j < count; ++j) delta_aggregate_block_wave<T>(a, first + j, lds, lane);
    });
}

typedef hipError_t (*delta_aggregate_launch_t)(const DeltaAggregateArgs&, int waves, hipStream_t);   // launch_block_consumer (fl_for_block.hpp)
template <typename T> delta_aggregate_launch_t delta_aggregate_launcher();

}  // namespace fl
