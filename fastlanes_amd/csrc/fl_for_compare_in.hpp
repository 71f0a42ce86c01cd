// fl_for_compare_in.hpp -- unfor_compare_in: set membership (WHERE x IN (...)) over a FoR-packed column, uniform or mixed width, chained
// through the mask so far.  EXTENSION, defined as a composition of reference functions; all arithmetic mod 2^T:
//     member(v)  = (j := (v - set_lo) mod 2^T) < set_bits  &&  bit j of set_words
//     hit[b][i]  = member(unfor_pack::<W_b>(block b, references[b * ref_stride])[i])  XOR  negate
//     NEW: mask[b] = hit[b]      AND: mask[b] = mask_in[b] & hit[b]      OR: mask[b] = mask_in[b] | hit[b]
// (ffor.rs:38-50; the masks in unpack_compare's layout, 32 words per block).  The set's window IS a ForPredicate (fl_set_decide.hpp), so
// this is k_unfor_compare_range (fl_for_compare_range.hpp) with one more step per element: the f + c the range kernel compares with s
// is the bitmap index j, `<= s` is the in-window test, and the hit is bit j of the bitmap.
//   * a block closed by its incoming mask, a block whose values all lie outside the window (for_compare_decide: FOR_CMP_NONE -- a miss,
//     or all-hit under negate) and a width-0 block (one bitmap bit) are answered WITHOUT a packed load (set_block_decide);
//   * REG, set_bits <= 2048 (fl_set_decide.hpp: SET_REGISTER_BITS): lane l keeps word l of the bitmap in a VGPR, loaded once per
//     wavefront through a descriptor sized to the words (lanes past them hold 0) and in flight with the first block's metadata; an
//     element's word is a cross-lane read (ds_bpermute_b32): no LDS allocation, no global gather;
//   * !REG, larger sets: one vector gather load per element, default (cached) policy, through a descriptor bounded to the bitmap's
//     bytes -- an index outside the window is given an offset past it, reads 0 and touches no memory; a block's 16 gathers per lane are
//     all in flight before the first is used;
//   * u8 / u16 cells are SWAR up to f + c; their elements are then extracted one by one for the lookup;
//   * a block that fails the mixed-width device checks is skipped: its FL_DEVERR_* bit is raised, its mask words are left alone.
// Every valid block's 128 bytes are always written; `mask` may be `mask_in` itself (as in unfor_compare_range).  Which tier a call takes
// is decided once on the host from set_bits.  LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_for_compare_range.hpp"
#include "fl_set_decide.hpp"

namespace fl {

// ForCompareArgs' predicate is the set's window: cmp_a = set_lo, cmp_s = set_bits - 1, cmp_none = (set_bits == 0)
struct ForInArgs : ForRangeArgs {
    const uint32_t* set_words;   // ceil(set_bits / 32) words; never read when set_bits == 0
    unsigned set_bytes;          // 4 * ceil(set_bits / 32) <= 2^29: the bitmap descriptor's size
    unsigned negate;             // 1: NOT IN
};

constexpr uint32_t SET_OUTSIDE = 0x80000000u;    // a byte offset past any bitmap (<= 2^29 bytes)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t set_descriptor(const ForInArgs& a)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(a.set_words), 0, a.set_bytes, 0x00020000);
}

// The bitmap word that holds bit j (j's low 32 bits: an index inside the window is < 2^32), 0 when j lies outside the window.
// REG: EVERY lane of the wavefront must get here (ds_bpermute_b32 reads from inactive lanes as 0).
template <bool REG>
__device__ __forceinline__ uint32_t set_word_of(const __amdgpu_buffer_rsrc_t& rs, uint32_t setw, uint32_t j, bool inside)
{
    if constexpr (REG) {
        const uint32_t w = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((j >> 3) & 252u), (int)setw);   // lane j / 32's word
        return inside ? w : 0u;
    } else {
        return __builtin_amdgcn_raw_buffer_load_b32(rs, inside ? (j >> 5) << 2 : SET_OUTSIDE, 0, 0);
    }
}

// The LDS image of an undecided block (1 <= w <= T rows) -> its verdicts: bit e of verdicts[k] = hit of element e of the lane's cell of
// group k.  16 elements per lane whatever the type: their words are all requested before the first is looked at.
template <typename T, bool REG>
__device__ __forceinline__ void in_image_verdicts(const ForInArgs& a, unsigned w, const char* lds, unsigned lane, T c, const __amdgpu_buffer_rsrc_t& rs,
                                                  uint32_t setw, uint32_t (&verdicts)[WaveBlock<T>::GROUPS])
{
    constexpr int N = Elem<T>::PER_CELL, GROUPS = WaveBlock<T>::GROUPS;
    const Cell<T> cc = Cell<T>::splat(c);
    const T s = (T)a.cmp_s;
    uint32_t word[GROUPS * N], at[GROUPS * N];
    for_each_funnelled_cell<T>(w, lds, lane, [&](auto K, unsigned bit, const Cell<T>& cell) {
        const Cell<T> j = cell.add(cc);                                     // (f + c) mod 2^T per element: the bitmap index
        static_for<N>([&](auto E) {
            constexpr int i = decltype(K)::value * N + decltype(E)::value;
            const T x = (T)cell_get<T>(j, decltype(E)::value);
            word[i] = set_word_of<REG>(rs, setw, (uint32_t)x, x <= s);
            at[i] = (uint32_t)x & 31u;
        });
    });
    const uint32_t flip = a.negate ? (1u << N) - 1u : 0u;
    static_for<GROUPS>([&](auto K) {
        uint32_t v = 0;
        static_for<N>([&](auto E) {
            constexpr int i = decltype(K)::value * N + decltype(E)::value;
            v |= ((word[i] >> at[i]) & 1u) << decltype(E)::value;
        });
        verdicts[decltype(K)::value] = v ^ flip;
    });
}

// The LDS image of an undecided block -> its mask: the verdict bits are gathered in the dead image (verdicts_to_image) and combined
// with `in` = the 16 bytes lanes base .. base + 7 hold of block `blk`'s mask_in, as combine_lds_image does
template <typename T, bool REG>
__device__ __forceinline__ void in_lds_image(const ForInArgs& a, uint64_t blk, unsigned w, char* lds, unsigned lane, T c, const __amdgpu_buffer_rsrc_t& rs,
                                             uint32_t setw, u32x4 in, unsigned base)
{
    uint32_t verdicts[WaveBlock<T>::GROUPS];
    in_image_verdicts<T, REG>(a, w, lds, lane, c, rs, setw, verdicts);
    verdicts_to_image<T>(verdicts, lds, lane);
    store_range_mask(a, blk, range_combine(a.combine, in, *reinterpret_cast<const u32x4*>(lds + (lane & 7u) * 16u)), lane, base);
}

// one block per call, as range_block_wave: metadata, reference and the incoming mask in flight together; only an open block requests
// its packed rows
template <typename T, bool REG>
__device__ __forceinline__ void in_block_wave(const ForInArgs& a, uint64_t blk, char* lds, unsigned lane, const __amdgpu_buffer_rsrc_t& rs, uint32_t setw)
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
    int verdict = set_block_decide(WaveBlock<T>::TB, predicate_of(a), m.r, m.w, c);
    if (verdict == SET_PROBE) {                                             // width 0 inside the window: bit c decides (c wave-uniform)
        uint32_t word;
        if constexpr (REG) word = (uint32_t)__builtin_amdgcn_readlane((int)setw, (int)(uint32_t)(c >> 5));
        else word = (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_amdgcn_raw_buffer_load_b32(rs, (uint32_t)(c >> 5) << 2, 0, 0));
        verdict = set_probe_verdict(word, c);
    }
    if (verdict != SET_EACH) {
        store_decided_range(a, blk, set_hit_verdict(verdict, a.negate != 0u), in, lane, 0u);
        return;
    }
    fill_block_image<T>(a, blk, m.off, m.w, lds, lane);
    in_lds_image<T, REG>(a, blk, m.w, lds, lane, (T)c, rs, setw, in, 0u);
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

// Several consecutive blocks per wavefront (the narrow types), as range_blocks_wave_prefetched: lane j judges block first + j --
// metadata, reference, preconditions, verdict, and for a width-0 block its one bitmap bit -- and lanes 8j .. 8j + 7 hold its incoming
// mask, BEFORE any packed load is issued; only the blocks still open are then requested by LDS-DMA, one image per block, one wait.
template <typename T, bool REG>
__device__ __forceinline__ void in_blocks_wave_prefetched(const ForInArgs& a, uint64_t first, unsigned count, char* lds, unsigned lane,
                                                          const __amdgpu_buffer_rsrc_t& rs, uint32_t setw)
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
    int vv = l.ev ? (int)SET_EACH : set_block_decide(G::TB, predicate_of(a), l.rv, l.wv, cv);
    if (__builtin_amdgcn_ballot_w64(vv == SET_PROBE) != 0ull) {           // wave-uniform: some width-0 block inside the window
        const uint32_t probe = set_word_of<REG>(rs, setw, (uint32_t)cv, vv == SET_PROBE);   // every lane: the lane's block's one bit
        if (vv == SET_PROBE) vv = set_probe_verdict(probe, cv);
    }
    vv = set_hit_verdict(vv, a.negate != 0u);
    // bit j: block first + j's answer is still open after its incoming mask (byte j % 8 of live[j / 8])
    unsigned open_blocks = 0;
    for (unsigned j = 0; j < count; ++j)                      // wave-uniform
        open_blocks |= (((live[j >> 3] >> (8u * (j & 7u))) & 0xffull) != 0ull ? 1u : 0u) << j;
    request_block_images<T>(a, l, __builtin_amdgcn_ballot_w64(l.owner && l.ev == 0u && vv == SET_EACH) & open_blocks, count, lds, lane);
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
        if (verdict != SET_EACH) {
            store_decided_range(a, blk, verdict, mi, lane, base);
            continue;
        }
        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)l.wv, (int)j);
        in_lds_image<T, REG>(a, blk, w, lds + j * G::BLOCK_BYTES, lane, (T)readlane_u64(cv, j), rs, setw, mi, base);
    }
}

template <typename T, bool REG>
__global__ __launch_bounds__(WG) void k_unfor_compare_in(ForInArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        const __amdgpu_buffer_rsrc_t rs = set_descriptor(a);
        uint32_t setw = 0;
        if constexpr (REG) setw = __builtin_amdgcn_raw_buffer_load_b32(rs, lane * 4u, 0, 0);   // <= 256 bytes; lanes past the words: 0
        if (a.prefetch && count > 1) {
            in_blocks_wave_prefetched<T, REG>(a, first, count, lds, lane, rs, setw);
            return;
        }
        for (unsigned j = 0; j < count; ++j) in_block_wave<T, REG>(a, first + j, lds, lane, rs, setw);
    });
}

typedef hipError_t (*for_in_launch_t)(const ForInArgs&, int waves, hipStream_t);   // launch_block_consumer (fl_for_block.hpp)
template <typename T> for_in_launch_t for_in_launcher(bool register_tier);

}  // namespace fl
