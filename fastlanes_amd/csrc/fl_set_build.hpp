// fl_set_build.hpp -- unfor_set_build: the member set of the values a FoR-packed column holds in the rows a selection mask keeps, built
// on the device (the BUILD side of the semi-join whose probe side is unfor_compare_in, fl_for_compare_in.hpp).  EXTENSION (SURVEY.md
// 8 f2), defined as a composition of reference functions; all arithmetic mod 2^T:
//     for every block b, every i with bit i of block b of `mask` set (mask == nullptr: every i):
//         v = unfor_pack::<W_b>(block b, references[b * ref_stride])[i]                                       (ffor.rs:38-50)
//         j = (v - set_lo) mod 2^T
//         j < set_bits:  bit j of set_words |= 1, inserted += 1          else:  outside += 1
//     stats[0] += inserted;  stats[1] += outside
// The call ORs and adds, it never clears: the caller zeroes set_words and stats or passes an earlier call's.  OR and integer add
// commute, so the result is bitwise reproducible.  The window is unfor_compare_in's (fl_set_decide.hpp), and with c = (r - set_lo) the
// f + c of the compare kernels is j.
// A run-walking kernel (fl_block_run.hpp: the run, the look-ahead, the stats tail; aggregate_lane_of, fl_aggregate.hpp, counts a lane's
// kept rows).  Per block, through the steps of fl_for_block.hpp: the route comes from fl_set_build_map.hpp (set_build_route): an empty
// mask reads nothing, a block outside the window and a width-0 block read no packed byte; every other block is decoded from its LDS
// image.  Two tiers, chosen once on the host from set_bits:
//   * SETB_LDS, set_bits <= SET_BUILD_LDS_BITS: a wave-private bitmap in LDS, zeroed at the start, updated with LDS atomic ORs that
//     return no value (two lanes of one instruction may hit one word), flushed at the wavefront's end -- only its non-zero words, with
//     global atomic ORs, the window's last word masked to set_bits;
//   * SETB_MEM / SETB_MEM_TEST, larger windows: one relaxed agent-scope vector atomic OR per kept in-window element straight into
//     set_words, no value returned; an index outside the window issues nothing (a branch, not a clamp).  SETB_MEM_TEST first loads the
//     word (cached, through a descriptor bounded to the bitmap) and issues the atomic only when the bit is still clear -- sound because
//     bits only ever turn on: a stale 0 costs one redundant atomic, a 1 is never stale.
// inserted / outside are counted per lane from the mask slices and the in-window tests (folded with wave_sum_u64, fl_block_run.hpp).  A block that fails the mixed-width device checks raises
// its FL_DEVERR_* bit and contributes nothing.  LDS is wave-local (in-order per wave): no s_barrier.  Every global store or atomic is
// a vector instruction.
#pragma once
#include "fl_aggregate.hpp"
#include "fl_set_build_map.hpp"

namespace fl {

enum SetBuildTier { SETB_LDS = 0, SETB_MEM = 1, SETB_MEM_TEST = 2 };

// WidthsArgs::refs and ::unpacked stay nullptr: the reference is loaded with the block's metadata
struct SetBuildArgs {
    WidthsArgs col;
    const void* refs;              // references[b * col.ref_stride]
    const uint32_t* mask;          // [n_blocks][32]; nullptr = every row is kept (no mask is read)
    uint32_t* set_words;           // ceil(set_bits / 32) words; never touched when set_bits == 0
    uint64_t* stats;               // {inserted, outside}; nullptr = not counted
    uint64_t cmp_a, cmp_s;         // the window as a ForPredicate: set_lo, set_bits - 1
    unsigned cmp_none;             // set_bits == 0
    unsigned n_words;              // ceil(set_bits / 32) <= 2^27
    uint32_t last_mask;            // the window's bits of its last word
    uint64_t run;                  // blocks of a wavefront's run; filled by the launcher
};

constexpr uint32_t SET_BUILD_PAST = 0x80000000u;  // a byte offset past any bitmap (<= 2^29 bytes)

template <typename T, int TIER> constexpr unsigned set_build_lds() { return set_build_wave_lds(WaveBlock<T>::BLOCK_BYTES, Elem<T>::BITS, TIER == SETB_LDS); }

// bit j (inside the window) of the bitmap: the wavefront's private one, or set_words itself
template <int TIER> __device__ __forceinline__ void set_build_bit(const SetBuildArgs& a, uint32_t* bitmap, uint32_t j)
{
    if constexpr (TIER == SETB_LDS) __hip_atomic_fetch_or(bitmap + (j >> 5), 1u << (j & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_or(a.set_words + (j >> 5), 1u << (j & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a block's loads, issued and possibly still in flight
template <typename T> struct SetBuildLoads {
    BlockLoads<T> m;
    uint32_t slice[SelectMap<sizeof(T)>::GROUPS];
};
template <typename T> __device__ __forceinline__ SetBuildLoads<T> set_build_issue(const SetBuildArgs& a, uint64_t blk, unsigned lane)
{
    SetBuildLoads<T> p;
    p.m = issue_block_loads<T>(a.col, a.refs, blk);
    block_mask_slices<T>(a.mask, blk, lane, p.slice);
    return p;
}

// The LDS image of an EACH block -> its bits; returns the lane's count of kept elements inside the window
template <typename T, int TIER>
__device__ __forceinline__ uint32_t set_build_image(const SetBuildArgs& a, unsigned w, const char* lds, uint32_t* bitmap, unsigned lane, T c,
                                                    const uint32_t (&slice)[SelectMap<sizeof(T)>::GROUPS])
{
    constexpr int N = Elem<T>::PER_CELL, GROUPS = WaveBlock<T>::GROUPS;
    const Cell<T> cc = Cell<T>::splat(c);
    const T s = (T)a.cmp_s;
    uint32_t inserted = 0;
    if constexpr (TIER == SETB_MEM_TEST) {
        // a block's 16 words per lane are all requested before the first is looked at, as the memory tier of unfor_compare_in gathers
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.set_words, 0, a.n_words * 4u, 0x00020000);
        uint32_t word[GROUPS * N], at[GROUPS * N];
        uint32_t inside = 0;                                                // bit i: element i is kept and inside the window
        for_each_funnelled_cell<T>(w, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) {
            const Cell<T> j = cell.add(cc);                                 // (f + c) mod 2^T per element: the bitmap index
            const uint32_t sl = slice[decltype(K)::value];
            static_for<N>([&](auto E) {
                constexpr int i = decltype(K)::value * N + decltype(E)::value;
                const T x = (T)cell_get<T>(j, decltype(E)::value);
                const bool in = ((sl >> decltype(E)::value) & 1u) != 0u && x <= s;
                word[i] = __builtin_amdgcn_raw_buffer_load_b32(rs, in ? ((uint32_t)x >> 5) << 2 : SET_BUILD_PAST, 0, 0);
                at[i] = (uint32_t)x;
                inside |= (in ? 1u : 0u) << i;
            });
        });
        static_for<GROUPS * N>([&](auto I) {
            constexpr int i = decltype(I)::value;
            if (((inside >> i) & 1u) != 0u && ((word[i] >> (at[i] & 31u)) & 1u) == 0u) set_build_bit<TIER>(a, bitmap, at[i]);
        });
        inserted = (uint32_t)__builtin_popcount(inside);
    } else {
        for_each_funnelled_cell<T>(w, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) {
            const Cell<T> j = cell.add(cc);                                 // (f + c) mod 2^T per element: the bitmap index
            const uint32_t sl = slice[decltype(K)::value];
            static_for<N>([&](auto E) {
                const T x = (T)cell_get<T>(j, decltype(E)::value);
                if (((sl >> decltype(E)::value) & 1u) != 0u && x <= s) {    // outside the window: nothing is issued
                    set_build_bit<TIER>(a, bitmap, (uint32_t)x);
                    ++inserted;
                }
            });
        });
    }
    return inserted;
}

// one block whose loads were issued by set_build_issue.  lds: [image | private bitmap (SETB_LDS)]; ins / out: the lane's counters
template <typename T, int TIER>
__device__ __forceinline__ void set_build_block(const SetBuildArgs& a, uint64_t blk, const SetBuildLoads<T>& p, char* lds, uint32_t* bitmap,
                                                unsigned lane, uint64_t& ins, uint64_t& out)
{
    const BlockMeta m = settle_block_loads<T>(a.col, blk, p.m);
    uint32_t any = 0;
    static_for<(int)SelectMap<sizeof(T)>::GROUPS>([&](auto K) { any |= p.slice[decltype(K)::value]; });
    const bool empty = __builtin_amdgcn_ballot_w64(any != 0u) == 0ull;
    if (m.err) raise_device_error(a.col.err_flag, m.err, lane);
    uint64_t c;
    const SetBuildRoute route = set_build_route(WaveBlock<T>::TB, ForPredicate{a.cmp_a, a.cmp_s, a.cmp_none != 0u}, empty, m.err == 0u, m.r, m.w, c);
    if (route == SETB_SKIP) return;
    const uint32_t kept = aggregate_lane_of<T>(p.slice).count;               // the lane's kept rows
    if (route == SETB_OUTSIDE) {
        out += kept;
        return;
    }
    if (route == SETB_ONE_BIT) {                                            // width 0 inside the window: bit c, c wave-uniform
        if (lane == 0u) set_build_bit<TIER>(a, bitmap, (uint32_t)c);
        ins += kept;
        return;
    }
    fill_block_image<T>(a.col, blk, m.off, m.w, lds, lane);
    const uint32_t inside = set_build_image<T, TIER>(a, m.w, lds, bitmap, lane, (T)c, p.slice);
    ins += inside;
    out += kept - inside;
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

// Workgroup (= wavefront) g owns blocks [g * run, (g + 1) * run) of the column; one that owns none returns at once and flushes nothing.
template <typename T, int TIER>
__global__ __launch_bounds__(64) void k_unfor_set_build(SetBuildArgs a)
{
    using G = WaveBlock<T>;
    extern __shared__ __attribute__((aligned(16))) char lds_all[];
    const unsigned lane = threadIdx.x;
    const uint64_t n = a.col.n_blocks;
    const uint64_t first = (uint64_t)blockIdx.x * a.run;
    if (first >= n) return;
    const uint64_t end = n - first < a.run ? n : first + a.run;
    uint32_t* bitmap = reinterpret_cast<uint32_t*>(lds_all + G::BLOCK_BYTES);
    if constexpr (TIER == SETB_LDS) {
        // whole 16-byte cells: n_words <= the private bitmap's words, which are a multiple of 4
        for (unsigned i = lane * 4u; i < a.n_words; i += 256u) *reinterpret_cast<u32x4*>(bitmap + i) = u32x4{0u, 0u, 0u, 0u};
        wave_lds_fence();
    }
    uint64_t ins = 0, out = 0;
    SetBuildLoads<T> cur = set_build_issue<T>(a, first, lane);
    for (uint64_t blk = first; blk < end; ++blk) {                          // wave-uniform loop
        const uint64_t ahead = blk + 1 < end ? blk + 1 : blk;               // the last block asks for itself again: straight-line code
        const SetBuildLoads<T> nxt = set_build_issue<T>(a, ahead, lane);
        set_build_block<T, TIER>(a, blk, cur, lds_all, bitmap, lane, ins, out);
        cur = nxt;
    }
    if constexpr (TIER == SETB_LDS) {
        wave_lds_fence();
        for (unsigned i = lane; i < a.n_words; i += 64u) {                  // as group_table_flush: only what this wavefront has set
            uint32_t word = bitmap[i];
            if (i == a.n_words - 1u) word &= a.last_mask;
            if (word != 0u) __hip_atomic_fetch_or(a.set_words + i, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (a.stats) {
        ins = wave_sum_u64(ins);
        out = wave_sum_u64(out);
        if (lane == 0u && ins != 0ull) __hip_atomic_fetch_add(a.stats, ins, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0u && out != 0ull) __hip_atomic_fetch_add(a.stats + 1, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <typename T, int TIER>
hipError_t launch_set_build(const SetBuildArgs& a, int waves, hipStream_t s)
{
    return launch_group_runs<k_unfor_set_build<T, TIER>, set_build_lds<T, TIER>()>(a, a.col.n_blocks, a.col.bpw, waves, s);
}

typedef hipError_t (*set_build_launch_t)(const SetBuildArgs&, int waves, hipStream_t);
template <typename T> set_build_launch_t set_build_launcher(int tier);

}  // namespace fl
