// fl_delta_compare_range.hpp -- undelta_compare_range: an interval predicate over a DELTA-packed column, uniform or mixed width, chained
// through the mask so far.  EXTENSION, defined as a composition of reference functions; all arithmetic mod 2^T:
//     v[b]      = untranspose(undelta_pack::<W_b>(block b, bases[b * LANES .. + LANES]))        (delta.rs:47-63, transpose.rs:17-22)
//     hit[b][i] = ((v[b][i] - lo) mod 2^T) <= ((hi - lo) mod 2^T)
//     NEW: mask[b] = hit[b]      AND: mask[b] = mask_in[b] & hit[b]      OR: mask[b] = mask_in[b] | hit[b]
// The masks are unfor_compare_range's (fl_for_compare_range.hpp): 32 words per block, bit i = ORIGINAL row i, LSB first; `mask` may be
// `mask_in` itself; every valid block's 128 bytes are always written.
// One wavefront per block, launched through the block-consumer plan as k_unfor_compare_range is:
//   * the block's width, offset, its 128 bytes of bases and its 128 bytes of mask_in are independent vector loads under one wait; lane
//     (i, c) holds the bases of cell column c (FL lanes N c .. N c + N - 1, N = 16 / sizeof(T)), so lanes 0..7 hold all of them;
//   * the route is fl_delta_compare_range_map.hpp's: SKIP (a device check failed), KEEP (the incoming mask decides), ALL / NONE / BASES
//     (fl_delta_decide.hpp, from cmin / cmax of c_l = base_l - a, reduced over the 8 lanes of a group by DPP) -- none of them requests a
//     packed byte -- and EACH;
//   * EACH fills the LDS image and takes the lane's R = T/8 consecutive rows through fl_chain.hpp's stages as they are
//     (chain_stage_source<SRC_PACKED, CHAIN_NONE>, chain_stage_rows<SRC_PACKED, CHAIN_UNDELTA>) with base - a as the base, so that each
//     element costs one unsigned compare against s.  No value is untransposed: lane (i, c) holds R verdict bits of each of its N FL
//     lanes, rows R i .. R i + R - 1 of that lane's T-bit group; the 8 lane groups' pieces are ORed together (ds_bpermute, 3 steps) and
//     lanes 0..7 place their N groups at bit lane_base(l) of the block's mask in the dead LDS image (u64: a lane's two groups ARE its 16
//     bytes of the mask, nothing is placed);
//   * the block leaves as ONE coalesced 128-byte store from lanes 0..7, combined with the incoming bytes just before it
//     (store_range_mask).
// LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_for_compare_range.hpp"
#include "fl_chain.hpp"
#include "fl_delta_compare_range_map.hpp"

namespace fl {

// ForRangeArgs::cmp_refs and ::ref_stride are unused: a Delta block has LANES bases, not one reference
struct DeltaRangeArgs : ForRangeArgs {
    const char* bases;         // [n_blocks][128 bytes]
};

// the packed side as fl_chain.hpp's stages read it; Args: any block-consumer argument block with Delta's `bases` beside it (this family's,
// undelta_aggregate's, undelta_select's)
template <typename Args> __device__ __forceinline__ ChainArgs chain_source_args(const Args& a)
{
    ChainArgs c;
    c.in = a.packed;
    c.out = nullptr;
    c.bases = a.bases;
    c.n_blocks = a.n_blocks;
    c.width = a.uniform_width;
    c.widths = a.widths;
    c.offsets = a.offsets;
    c.err_flag = a.err_flag;
    c.packed_bytes = a.packed_bytes;
    c.nt_from = a.nt_from;
    return c;
}

// min / max of x over the 8 lanes of a lane group (every lane of the group receives them); full wave
__device__ __forceinline__ uint64_t group_partner_u64(uint64_t x, int step)
{
    const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    const uint32_t plo = step == 0 ? butterfly_partner<0>(lo) : step == 1 ? butterfly_partner<1>(lo) : butterfly_partner<2>(lo);
    const uint32_t phi = step == 0 ? butterfly_partner<0>(hi) : step == 1 ? butterfly_partner<1>(hi) : butterfly_partner<2>(hi);
    return ((uint64_t)phi << 32) | plo;
}
template <typename T> __device__ __forceinline__ void group_min_max(const Cell<T>& c, uint64_t& cmin, uint64_t& cmax)
{
    constexpr int N = Elem<T>::PER_CELL;
    uint64_t lo = cell_get<T>(c, 0), hi = lo;
    static_for<N - 1>([&](auto E) {
        const uint64_t v = cell_get<T>(c, decltype(E)::value + 1);
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    });
    static_for<3>([&](auto S) {
        const uint64_t pl = sizeof(T) == 8 ? group_partner_u64(lo, decltype(S)::value) : (uint64_t)(uint32_t)group_partner_u64(lo, decltype(S)::value);
        const uint64_t ph = sizeof(T) == 8 ? group_partner_u64(hi, decltype(S)::value) : (uint64_t)(uint32_t)group_partner_u64(hi, decltype(S)::value);
        lo = pl < lo ? pl : lo;
        hi = ph > hi ? ph : hi;
    });
    cmin = wave_uniform_u64(lo);
    cmax = wave_uniform_u64(hi);
}

// The lane's 128 bits of verdict groups: group e (FL lane N c + e) occupies bits e T .. e T + T - 1 of v[0..3].
// BASES: every row of chain e answers bit e of `bits`
template <typename T> __device__ __forceinline__ void groups_of_bases(uint32_t bits, uint32_t (&v)[4])
{
    constexpr int TB = WaveBlock<T>::TB, N = Elem<T>::PER_CELL;
    for (int k = 0; k < 4; ++k) v[k] = 0u;
    static_for<N>([&](auto E) {
        constexpr int e = decltype(E)::value;
        const uint32_t all = 0u - ((bits >> e) & 1u);
        if constexpr (TB == 64) {
            v[2 * e] = all;
            v[2 * e + 1] = all;
        } else if constexpr (TB == 32) {
            v[e] = all;
        } else {
            v[(e * TB) >> 5] |= (all & ((1u << TB) - 1u)) << ((e * TB) & 31);
        }
    });
}
// EACH: rows[j] = bit e <-> element e of the lane's row R i + j; the lane's piece of group e is bits R i .. R i + R - 1 of it
template <typename T> __device__ __forceinline__ void groups_of_rows(const uint32_t (&rows)[WaveBlock<T>::TB / 8], unsigned i, uint32_t (&v)[4])
{
    constexpr int TB = WaveBlock<T>::TB, R = TB / 8, N = Elem<T>::PER_CELL;
    for (int k = 0; k < 4; ++k) v[k] = 0u;
    static_for<R>([&](auto J) {
        static_for<N>([&](auto E) {
            constexpr int pos = decltype(E)::value * TB + decltype(J)::value;
            v[pos >> 5] |= ((rows[decltype(J)::value] >> decltype(E)::value) & 1u) << (pos & 31);
        });
    });
    if constexpr (TB == 64) {
        for (int e = 0; e < 2; ++e) {
            const uint64_t g = (uint64_t)v[2 * e] << (8u * i);
            v[2 * e] = (uint32_t)g;
            v[2 * e + 1] = (uint32_t)(g >> 32);
        }
    } else {
        for (int k = 0; k < 4; ++k) v[k] <<= (unsigned)R * i;              // R i + R <= T: a piece stays inside its group
    }
}
// OR over the 8 lane groups (lanes c, c + 8, .., c + 56); every lane receives the result
__device__ __forceinline__ void or_over_lane_groups(uint32_t (&v)[4], unsigned lane)
{
    static_for<3>([&](auto S) {
        const int partner = (int)((lane ^ (8u << decltype(S)::value)) * 4u);
        for (int k = 0; k < 4; ++k) v[k] |= (uint32_t)__builtin_amdgcn_ds_bpermute(partner, (int)v[k]);
    });
}
// Lanes 0..7 hold the groups of FL lanes N lane .. N lane + N - 1 -> the 16 bytes lane (lane & 7) stores of the block's mask.  The
// wavefront's LDS image must be dead (its first 128 bytes are used); u64 touches no LDS: FL lane l's group is bytes 8 l .. 8 l + 7.
template <typename T> __device__ __forceinline__ u32x4 place_groups(const uint32_t (&v)[4], char* lds, unsigned lane)
{
    constexpr int TB = WaveBlock<T>::TB, N = Elem<T>::PER_CELL;
    if constexpr (TB == 64) {
        return u32x4{v[0], v[1], v[2], v[3]};
    } else {
        if (lane < 8u) {
            static_for<N>([&](auto E) {
                constexpr int e = decltype(E)::value;
                char* at = lds + delta_group_bit((unsigned)N * lane + e) / 8u;
                if constexpr (TB == 32) *reinterpret_cast<uint32_t*>(at) = v[e];
                else if constexpr (TB == 16) *reinterpret_cast<uint16_t*>(at) = (uint16_t)(v[e >> 1] >> (16 * (e & 1)));
                else *reinterpret_cast<uint8_t*>(at) = (uint8_t)(v[e >> 2] >> (8 * (e & 3)));
            });
        }
        wave_lds_fence();
        return *reinterpret_cast<const u32x4*>(lds + (lane & 7u) * 16u);
    }
}

// one block per call
template <typename T>
__device__ __forceinline__ void delta_range_block_wave(const DeltaRangeArgs& a, uint64_t blk, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    constexpr int TB = G::TB, R = TB / 8;
    // width, offset, bases and the incoming mask: independent vector loads, one wait
    const unsigned z = opaque_zero();
    unsigned wv = a.uniform_width;
    uint64_t ov = 0;
    if (a.widths) wv = a.widths[blk + z];
    if (a.offsets) ov = a.offsets[blk + z];
    const Cell<T> base = __builtin_bit_cast(Cell<T>, *reinterpret_cast<const u32x4*>(a.bases + blk * 128u + (lane & 7u) * 16u + z));
    u32x4 in = {0u, 0u, 0u, 0u};
    if (a.combine != MASK_NEW) {
        // exactly this block's 128 bytes: lanes 8..63 read past the descriptor, which returns 0 and touches no memory
        const __amdgpu_buffer_rsrc_t ms = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.mask_in) + blk * 128u, 0, 128u, 0x00020000);
        in = __builtin_amdgcn_raw_buffer_load_b128(ms, lane * 16u, 0, 0);
    }
    const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(wv);
    const uint64_t off = a.offsets ? wave_uniform_u64(ov) : blk * (uint64_t)(128u * w);
    if (const uint32_t e = block_precondition(a, w, off, TB)) {                 // SKIP
        raise_device_error(a.err_flag, e, lane);
        return;
    }
    if (__builtin_amdgcn_ballot_w64(lane < 8u && range_mask_live(a.combine, in)) == 0ull) {
        store_range_mask(a, blk, in, lane, 0u);                                 // KEEP: mask_in is the answer
        return;
    }
    const Cell<T> cb = base.sub(Cell<T>::splat((T)a.cmp_a));                    // c_l = (base_l - a) mod 2^T
    uint64_t cmin, cmax;
    group_min_max<T>(cb, cmin, cmax);
    const int verdict = delta_compare_decide(TB, predicate_of(a), cmin, cmax, w);
    if (verdict == DELTA_CMP_ALL || verdict == DELTA_CMP_NONE) {
        store_decided_range(a, blk, verdict, in, lane, 0u);
        return;
    }
    const T s = (T)a.cmp_s;
    uint32_t v[4];
    if (verdict == DELTA_CMP_BASES) {                                           // W = 0: each chain repeats its base
        groups_of_bases<T>(row_predicate_bits<T, TB, false>(cb, s), v);
    } else {
        const ChainArgs ca = chain_source_args(a);
        Cell<T> unused;
        chain_stage_source<T, SRC_PACKED, CHAIN_NONE, RD_AUTO>(ca, blk, w, off, lds, lane, unused);
        wave_lds_fence();
        Cell<T> x[R];
        chain_stage_rows<T, SRC_PACKED, CHAIN_UNDELTA>(w, lds, lane, cb, x);
        uint32_t rows[R];
        static_for<R>([&](auto J) { rows[decltype(J)::value] = row_predicate_bits<T, TB, false>(x[decltype(J)::value], s); });
        groups_of_rows<T>(rows, lane >> 3, v);
        or_over_lane_groups(v, lane);
        wave_lds_fence();                                                       // every lane holds its rows: the image is dead
    }
    const u32x4 hit = place_groups<T>(v, lds, lane);
    store_range_mask(a, blk, range_combine(a.combine, in, hit), lane, 0u);
    wave_lds_fence();                                                           // the image is reused by the wavefront's next block
}

template <typename T>
__global__ __launch_bounds__(WG) void k_undelta_compare_range(DeltaRangeArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        for (unsigned j = 0; j < count; ++j) delta_range_block_wave<T>(a, first + j, lds, lane);
    });
}

typedef hipError_t (*delta_range_launch_t)(const DeltaRangeArgs&, int waves, hipStream_t);   // launch_block_consumer (fl_for_block.hpp)
template <typename T> delta_range_launch_t delta_range_launcher();

}  // namespace fl
