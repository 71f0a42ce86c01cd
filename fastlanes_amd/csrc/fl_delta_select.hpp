// fl_delta_select.hpp -- undelta_select: decode only the rows a selection mask keeps, from a DELTA-packed column, uniform or mixed width.
// EXTENSION (SURVEY.md 8 f2 "unpack -> filter" / f4 "take"), defined as a composition of reference functions; arithmetic mod 2^T:
//     v[b] = untranspose(undelta_pack::<W_b>(block b, bases[b * LANES .. + LANES]))              (delta.rs:47-63, transpose.rs:17-22)
//     out  = concat over b ascending of [ v[b][i]  for i ascending if bit i of block b of mask ]
// The mask is the one every compare entry point writes and undelta_compare_range produces: 32 words per block, bit i = ORIGINAL row i,
// LSB first.  Block b's run starts at out + out_offsets[b] (elements); out_offsets / total are fl_mask_offsets' (fl_scan.hpp), and
// everything else is unfor_select's contract (fl_select.hpp): a block that fails a device check is skipped with its output slots
// untouched, a block whose run does not lie inside [0, out_len) is skipped with FL_DEVERR_BOUNDS, err_flag serves the uniform form too.
// It rests on the lane-group fact of fl_delta_compare_range_map.hpp: the T chained rows of FastLanes lane l are the T consecutive
// original rows lane_base(l) .. + T - 1, so the mask bits that govern one chain are the aligned T-bit group at bit delta_group_bit(l),
// and a kept row's place in the run is a popcount over the mask (fl_delta_select_map.hpp), known before a packed byte arrives: the
// chains are compacted where they are decoded and no value is untransposed.
// One wavefront per block, launched through the block-consumer plan as k_undelta_aggregate is:
//   * the block's width, offset, its 128 bytes of bases, its 128 bytes of mask and out_offsets[b] are independent vector loads under one
//     wait; lane (i, c) holds the bases of cell column c (FL lanes N c .. N c + N - 1, N = 16 / sizeof(T));
//   * the route is fl_delta_select_map.hpp's: SKIP (a device check failed: the bit is raised), EMPTY (an all-zero mask), BOUNDS (the run
//     is not inside `out`), BASES (W = 0) -- none of them requests a packed byte -- and EACH;
//   * the lane's mask bits and landings: lane_mask_groups (fl_delta_aggregate.hpp) stages the mask's 128 bytes in the still unused LDS
//     image and hands every lane the N groups of its cell column; lanes 0..31 then take one mask word each, ONE wave scan of their
//     popcounts gives every word's exclusive prefix and the block's count, {prefix, word} pairs are staged behind the mask and every lane
//     reads the pair of each of its groups: group prefix = the word's prefix + the bits of the word below the group (u8 / u16; a u32
//     group starts its word).  A fence and a wait that retires these reads (the fill may be LDS-DMA, which LDS order does not
//     cover), and only then is the image filled.  u64: a lane's two groups ARE 16 bytes of the mask, which
//     every lane loads itself; the scan runs over the 8 lanes of a lane group and nothing is staged;
//   * EACH fills the LDS image and takes the lane's R = T/8 consecutive rows through fl_chain.hpp's stages as they are
//     (chain_stage_source<SRC_PACKED, CHAIN_NONE>, chain_stage_rows<SRC_PACKED, CHAIN_UNDELTA>): lane (i, c) holds rows R i .. R i + R - 1
//     of its N chains, 16 elements for every type.  After a fence the image is dead, and element e of row R i + j, if its bit of
//     lane_piece_bits is set, is written straight from its register to run[group prefix + popcount(group_e below row R i + j)] in that
//     same image (1024 elements: BLOCK_BYTES) -- no original-order image, no second LDS region;
//   * BASES writes from the bases through the same landing map: every row of a chain is its base;
//   * after another fence the run leaves as select_lds_image sends it: one element per lane per store, a wave-uniform trip count, a
//     descriptor of exactly count * sizeof(T) bytes -- the destination is only element-aligned and the neighbouring bytes belong to
//     other wavefronts.
// LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_select.hpp"
#include "fl_delta_aggregate.hpp"
#include "fl_delta_select_map.hpp"

namespace fl {

// SelectArgs::sel_refs and ::ref_stride are unused: a Delta block has LANES bases, not one reference
struct DeltaSelectArgs : SelectArgs {
    const char* bases;         // [n_blocks][128 bytes]
};

// Every LDS read the wavefront has issued has returned.  wave_lds_fence orders the compiler's LDS accesses and emits no wait, and LDS
// operations of one wavefront run in order among themselves -- but LDS-DMA writes the image from the memory side, unordered against
// them: before an image whose bytes were just READ is filled by LDS-DMA, the reads must have retired.
__device__ __forceinline__ void wave_lds_reads_retired() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// whole group e of lane_mask_groups' layout: bit r = row r of FL lane N c + e
template <typename T> __device__ __forceinline__ uint64_t lane_group(const uint32_t (&v)[4], int e)
{
    constexpr int TB = WaveBlock<T>::TB;
    if constexpr (TB == 64) return ((uint64_t)v[2 * e + 1] << 32) | v[2 * e];
    else if constexpr (TB == 32) return v[e];
    else return (v[(e * TB) >> 5] >> ((e * TB) & 31)) & ((1u << TB) - 1u);
}

// The prefixes of the lane's N groups (the mask bits of the block below each) and the block's count (wave-uniform), from one scan of the
// 32 words' popcounts.  `in` as lane_mask_groups takes it.  Narrower than u64: the mask stands in the first 128 bytes of the wavefront's
// LDS image (lane_mask_groups put it there), the {prefix, word} pairs go into the 256 bytes behind it, and the image must still be unused.
template <typename T>
__device__ __forceinline__ void lane_group_prefixes(const u32x4& in, char* lds, unsigned lane, unsigned (&prefix)[Elem<T>::PER_CELL], unsigned& count)
{
    constexpr int TB = WaveBlock<T>::TB, N = Elem<T>::PER_CELL;
    if constexpr (TB == 64) {
        const unsigned lo = (unsigned)(__builtin_popcount(in[0]) + __builtin_popcount(in[1]));
        const unsigned mine = lo + (unsigned)(__builtin_popcount(in[2]) + __builtin_popcount(in[3]));
        unsigned incl = mine;                                                   // lanes c, c + 8, .. hold the same 16 bytes: 8-lane scans
        for (int d = 1; d < 8; d <<= 1) {
            const unsigned o = __shfl_up(incl, d, 8);
            if ((lane & 7u) >= (unsigned)d) incl += o;
        }
        prefix[0] = incl - mine;
        prefix[1] = incl - mine + lo;
        count = (unsigned)__builtin_amdgcn_readlane((int)incl, 7);
    } else {
        const uint32_t word = *reinterpret_cast<const uint32_t*>(lds + (lane & 31u) * 4u);
        const uint32_t mine = lane < 32u ? (uint32_t)__builtin_popcount(word) : 0u;
        const uint32_t incl = select_wave_incl_scan<uint32_t>(mine, lane);
        count = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
        if (lane < 32u) *reinterpret_cast<select_u32x2*>(lds + 128u + lane * 8u) = select_u32x2{incl - mine, word};
        wave_lds_fence();
        static_for<N>([&](auto E) {
            constexpr int e = decltype(E)::value;
            const unsigned gb = delta_group_bit((unsigned)N * (lane & 7u) + e);
            const char* at = lds + 128u + (gb >> 5) * 8u;
            if constexpr (TB == 32) {
                prefix[e] = *reinterpret_cast<const uint32_t*>(at);             // a u32 group starts its word
            } else {
                const select_u32x2 pw = *reinterpret_cast<const select_u32x2*>(at);
                prefix[e] = delta_select_group_prefix(pw[0], pw[1], gb);
            }
        });
        wave_lds_fence();                                                       // the reads are issued; the caller retires them before an LDS-DMA fill
    }
}

// one block per call
template <typename T>
__device__ __forceinline__ void delta_select_block_wave(const DeltaSelectArgs& a, uint64_t blk, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    constexpr int TB = G::TB, R = TB / 8, N = Elem<T>::PER_CELL;
    static_assert(G::BLOCK_BYTES >= 128 + 256, "the mask and the {prefix, word} pairs are staged in the image");
    // width, offset, bases, the mask and out_offsets[b]: independent vector loads, one wait
    const unsigned z = opaque_zero();
    unsigned wv = a.uniform_width;
    uint64_t ov = 0;
    if (a.widths) wv = a.widths[blk + z];
    if (a.offsets) ov = a.offsets[blk + z];
    const uint64_t dv = a.out_offsets[blk + z];
    const Cell<T> base = __builtin_bit_cast(Cell<T>, *reinterpret_cast<const u32x4*>(a.bases + blk * 128u + (lane & 7u) * 16u + z));
    // exactly this block's 128 bytes: a lane that reads past the descriptor receives 0 and touches no memory
    const __amdgpu_buffer_rsrc_t ms = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(a.mask) + blk * 32u, 0, 128u, 0x00020000);
    const u32x4 in = __builtin_amdgcn_raw_buffer_load_b128(ms, (TB == 64 ? (lane & 7u) : lane) * 16u, 0, 0);
    const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(wv);
    const uint64_t off = a.offsets ? wave_uniform_u64(ov) : blk * (uint64_t)(128u * w);
    const uint64_t dst = wave_uniform_u64(dv);
    if (const uint32_t e = block_precondition(a, w, off, TB)) {                 // SKIP
        raise_device_error(a.err_flag, e, lane);
        return;
    }
    if (__builtin_amdgcn_ballot_w64(lane < 8u && (in[0] | in[1] | in[2] | in[3]) != 0u) == 0ull) return;   // EMPTY
    uint32_t v[4];
    lane_mask_groups<T>(in, lds, lane, v);
    unsigned prefix[N], count;
    lane_group_prefixes<T>(in, lds, lane, prefix, count);
    if (!select_run_inside(a, dst, count)) {                                    // BOUNDS
        raise_device_error(a.err_flag, DEVERR_BOUNDS, lane);
        return;
    }
    Cell<T> x[R];
    if (w == 0u) {                                                              // BASES: each chain repeats its base
        static_for<R>([&](auto J) { x[decltype(J)::value] = base; });
    } else {                                                                    // EACH
        const ChainArgs ca = chain_source_args(a);
        Cell<T> unused;
        wave_lds_reads_retired();                                               // the staged mask and pairs (the run of the block before) were read: the fill may be LDS-DMA
        chain_stage_source<T, SRC_PACKED, CHAIN_NONE, RD_AUTO>(ca, blk, w, off, lds, lane, unused);
        wave_lds_fence();
        chain_stage_rows<T, SRC_PACKED, CHAIN_UNDELTA>(w, lds, lane, base, x);
        wave_lds_fence();                                                       // every lane holds its rows: the image is dead
    }
    // rows R i .. R i + R - 1 of chain e land one behind the other: bit e R + j of `bits` <-> element e of row R i + j
    const unsigned i = lane >> 3;
    const uint32_t bits = lane_piece_bits<T>(v, i);
    T* run = reinterpret_cast<T*>(lds);
    static_for<N>([&](auto E) {
        constexpr int e = decltype(E)::value;
        unsigned at = delta_select_landing(prefix[e], lane_group<T>(v, e), (unsigned)R * i);
        static_for<R>([&](auto J) {
            constexpr int j = decltype(J)::value;
            const unsigned on = (bits >> (e * R + j)) & 1u;
            if (on) run[at] = (T)cell_get<T>(x[j], e);                          // at < count <= 1024: inside the image
            at += on;
        });
    });
    wave_lds_fence();
    // exactly this block's count * sizeof(T) bytes: lanes past the run's end are dropped by the descriptor
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.out + dst * sizeof(T), 0, count * (unsigned)sizeof(T), 0x00020000);
    for (unsigned i0 = 0; i0 < count; i0 += 64u) {                              // wave-uniform trip count; i0 + lane < 1024: inside the image
        const unsigned k = i0 + lane;
        select_store_elem<T>(run[k], rs, k * (unsigned)sizeof(T));
    }
    wave_lds_fence();                                                           // the image is reused by the wavefront's next block
}

template <typename T>
__global__ __launch_bounds__(WG) void k_undelta_select(DeltaSelectArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        for (unsigned j = 0; j < count; ++j) delta_select_block_wave<T>(a, first + j, lds, lane);
    });
}

typedef hipError_t (*delta_select_launch_t)(const DeltaSelectArgs&, int waves, hipStream_t);   // launch_block_consumer (fl_for_block.hpp)
template <typename T> delta_select_launch_t delta_select_launcher();

}  // namespace fl
