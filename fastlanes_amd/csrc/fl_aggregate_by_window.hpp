// fl_aggregate_by_window.hpp -- unfor_aggregate_by_window: COUNT / SUM / MIN / MAX of a FoR-packed VALUE column grouped by a FoR-packed
// KEY column of the SAME element type and block count inside a dense window of the key domain, over the rows a selection mask keeps
// (GROUP BY l_orderkey, o_custkey, l_suppkey, ...: keys wider than unfor_aggregate_by's u8).  EXTENSION, defined as a
// composition of reference functions; all key arithmetic mod 2^T:
//     for every block b, every i with bit i of block b of `mask` set (mask == nullptr: every i):
//         val = unfor_pack::<W_b >(value block b, references[b * ref_stride])[i]                  zero-extended      (ffor.rs:38-50)
//         key = unfor_pack::<KW_b>(key block b, key_references[b * key_ref_stride])[i]
//         j   = (key - key_lo) mod 2^T
//         j < n_groups:  counts[j] += 1, sums[j] += val, mins[j] = min(mins[j], val), maxs[j] = max(maxs[j], val), inside += 1
//         else:          outside += 1
//     stats[0] += inside;  stats[1] += outside
// The call accumulates, it never clears: the caller writes the identities 0 / 0 / UINT64_MAX / 0 or passes an earlier call's arrays.  An
// array that is nullptr is not maintained; when sums, mins and maxs are all nullptr no packed byte of the value column is requested (the
// value width is taken as 0, ONE wave-uniform select per block).  Integer add, min and max commute: the result is bitwise reproducible.
// The window is unfor_set_build's (fl_set_decide.hpp), and with c = (key reference - key_lo) the f + c of the compare kernels is j.
// A run-walking kernel (fl_block_run.hpp: the run, the look-ahead, the wave-private table and its flush, the stats tail, the fetch of
// two columns through ONE image).  Per block, through the steps of fl_for_block.hpp: both columns' preconditions are checked; the route
// comes from fl_aggregate_by_window_map.hpp (aggregate_by_window_route): an empty mask reads nothing, a key block outside the window
// reads neither column, a width-0 key block inside it is unfor_aggregate's block folded into slot c.  Every other block fetches both
// columns under ONE wait -- the key rows into the wavefront's image, the value rows into staging registers; the lane keeps its 16 / N
// cells of j = f + c in registers, then the staged value rows are funnelled in the same lane map.  No key area.
// Two tiers, chosen once on the host from n_groups:
//   * AGGW_LDS, n_groups <= AGGREGATE_BY_WINDOW_LDS_GROUPS: the wave-private table, only the window's slots initialised, flushed only
//     into the arrays that are not nullptr;
//   * AGGW_MEM, larger windows: one relaxed agent-scope 64-bit vector atomic per kept in-window element and non-null array straight into
//     counts[j] / sums[j] / mins[j] / maxs[j], no value returned; a key outside the window issues nothing (a branch, not a clamp).
// inside / outside are counted per lane (folded with wave_sum_u64, fl_block_run.hpp).  A block that fails the mixed-width device checks of either column raises its
// FL_DEVERR_* bits and contributes nothing.  LDS is wave-local (in-order per wave): no s_barrier.  Every global store or atomic is a
// vector instruction.
#pragma once
#include "fl_aggregate.hpp"
#include "fl_aggregate_by_window_map.hpp"

namespace fl {

enum AggregateByWindowTier { AGGW_LDS = 0, AGGW_MEM = 1 };

// WidthsArgs::refs and ::unpacked stay nullptr in both columns: the references are loaded with the blocks' metadata
struct AggregateByWindowArgs {
    WidthsArgs val, key;           // the same n_blocks, the same err_flag
    const void* val_refs;          // references[b * val.ref_stride]
    const void* key_refs;          // key_references[b * key.ref_stride]
    const uint32_t* mask;          // [n_blocks][32]; nullptr = every row is kept (no mask is read)
    uint64_t* counts;              // [n_groups] each; nullptr = not maintained
    uint64_t* sums;
    uint64_t* mins;
    uint64_t* maxs;
    uint64_t* stats;               // {inside, outside}; nullptr = not counted
    uint64_t cmp_a, cmp_s;         // the window as a ForPredicate: key_lo, n_groups - 1
    unsigned cmp_none;             // n_groups == 0
    unsigned need_values;          // sums, mins or maxs is maintained: the value column is decoded
    unsigned n_slots;              // AGGW_LDS: n_groups, the slots of the private table in use
    uint64_t run;                  // blocks of a wavefront's run; filled by the launcher
};

template <typename T, int TIER> constexpr unsigned aggregate_by_window_lds() { return aggregate_by_window_wave_lds(WaveBlock<T>::BLOCK_BYTES, TIER == AGGW_LDS); }

// the arrays' slot j <- one partial aggregate: no-return 64-bit vector atomics, only into the arrays the caller maintains
__device__ __forceinline__ void window_arrays_update(const AggregateByWindowArgs& a, uint64_t j, uint64_t count, uint64_t sum, uint64_t lo, uint64_t hi)
{
    if (a.counts) __hip_atomic_fetch_add(a.counts + j, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.sums) __hip_atomic_fetch_add(a.sums + j, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.mins) __hip_atomic_fetch_min(a.mins + j, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.maxs) __hip_atomic_fetch_max(a.maxs + j, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// slot j (inside the window) of the wavefront's private table, or of the arrays themselves
template <int TIER>
__device__ __forceinline__ void window_slot_update(const AggregateByWindowArgs& a, BlockAggregate* table, uint64_t j, uint64_t count, uint64_t sum,
                                                   uint64_t lo, uint64_t hi)
{
    if constexpr (TIER == AGGW_LDS) group_table_update(table, (unsigned)j, count, sum, lo, hi);
    else window_arrays_update(a, j, count, sum, lo, hi);
}

// a block's loads, issued and possibly still in flight.  Args: AggregateByWindowArgs, or unfor_aggregate_by_lookup's, which names the two
// columns, their references and the mask alike
template <typename T> struct WindowBlockLoads {
    BlockLoads<T> v, k;
    uint32_t slice[SelectMap<sizeof(T)>::GROUPS];
};
template <typename T, typename Args> __device__ __forceinline__ WindowBlockLoads<T> aggregate_by_window_issue(const Args& a, uint64_t blk, unsigned lane)
{
    WindowBlockLoads<T> p;
    p.v = issue_block_loads<T>(a.val, a.val_refs, blk);
    p.k = issue_block_loads<T>(a.key, a.key_refs, blk);
    block_mask_slices<T>(a.mask, blk, lane, p.slice);
    return p;
}

// one block whose loads were issued by aggregate_by_window_issue.  lds: [image | private table (AGGW_LDS)]; ins / out: the lane's counters
template <typename T, int TIER>
__device__ __forceinline__ void aggregate_by_window_block(const AggregateByWindowArgs& a, uint64_t blk, const WindowBlockLoads<T>& p, char* lds,
                                                          BlockAggregate* table, unsigned lane, uint64_t& ins, uint64_t& out)
{
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    static_assert(M::GROUPS == (unsigned)G::GROUPS && M::N == (unsigned)Elem<T>::PER_CELL, "fl_select_map.hpp follows fl_widths.hpp's lane map");
    const BlockMeta mv = settle_block_loads<T>(a.val, blk, p.v);
    const BlockMeta mk = settle_block_loads<T>(a.key, blk, p.k);
    uint32_t any = 0;
    static_for<(int)M::GROUPS>([&](auto K) { any |= p.slice[decltype(K)::value]; });
    const bool empty = __builtin_amdgcn_ballot_w64(any != 0u) == 0ull;
    const uint32_t err = mv.err | mk.err;
    if (err) raise_device_error(a.val.err_flag, err, lane);
    uint64_t c;
    const AggregateByWindowRoute route =
        aggregate_by_window_route(G::TB, ForPredicate{a.cmp_a, a.cmp_s, a.cmp_none != 0u}, empty, err == 0u, mk.r, mk.w, c);
    if (route == AGGW_SKIP) return;
    const uint32_t kept = aggregate_lane_of<T>(p.slice).count;               // the lane's kept rows
    if (route == AGGW_OUTSIDE) {
        out += kept;
        return;
    }
    const T r = (T)mv.r;
    const unsigned vw = a.need_values != 0u ? mv.w : 0u;                    // counts alone: the value block is its reference, no byte of it is requested
    if (route == AGGW_ONE_GROUP) {                                          // unfor_aggregate's block, folded into slot c (c wave-uniform)
        BlockAggregate g;
        if (vw == 0u) {
            g = aggregate_constant_block(aggregate_wave_count(kept), (uint64_t)r);
        } else {
            fill_block_image<T>(a.val, blk, mv.off, vw, lds, lane);
            g = aggregate_lds_image<T>(vw, lds, lane, r, p.slice);
            wave_lds_fence();                                               // the image is reused by the wavefront's next block
        }
        if (lane == 0u) window_slot_update<TIER>(a, table, c, g.count, g.sum, g.min, g.max);
        ins += kept;
        return;
    }
    // both columns under one wait: wave-uniform descriptors over exactly each block's bytes (a width-0 value block: none); the key rows
    // (1 <= key width <= T) by LDS-DMA into the image, the value rows into staging registers
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.key.packed) + mk.off, 0, 128u * mk.w, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.val.packed) + mv.off, 0, 128u * vw, 0x00020000);
    const StagedRows<T> pk = request_image_and_staged<T>(krs, mk.w, vrs, vw, lds, lane);
    wait_lds_dma();
    wave_lds_fence();
    // the key block: the lane's slots j = f + c into registers
    Cell<T> kj[G::GROUPS];
    const Cell<T> cc = Cell<T>::splat((T)c);
    for_each_funnelled_cell<T>(mk.w, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) { kj[decltype(K)::value] = cell.add(cc); });
    staged_to_image<T>(pk, vw, lds, lane);
    // the value block through the same lane map (vw = 0: every field is 0, the value is the reference)
    const Cell<T> rc = Cell<T>::splat(r);
    const T s = (T)a.cmp_s;
    uint32_t inside = 0;
    for_each_funnelled_cell<T>(vw, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) {
        constexpr int k = decltype(K)::value;
        const Cell<T> v = cell.add(rc);                                     // ffor.rs:46-48
        const uint32_t sl = p.slice[k];
        static_for<(int)M::N>([&](auto E) {
            constexpr int e = decltype(E)::value;
            const T j = (T)cell_get<T>(kj[k], e);
            if (((sl >> e) & 1u) != 0u && j <= s) {                         // outside the window: nothing is issued
                const uint64_t x = (uint64_t)cell_get<T>(v, e);
                window_slot_update<TIER>(a, table, (uint64_t)j, 1ull, x, x, x);
                ++inside;
            }
        });
    });
    ins += inside;
    out += kept - inside;
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

// Workgroup (= wavefront) g owns blocks [g * run, (g + 1) * run) of the column; one that owns none returns before it touches LDS.
template <typename T, int TIER>
__global__ __launch_bounds__(64) void k_unfor_aggregate_by_window(AggregateByWindowArgs a)
{
    using G = WaveBlock<T>;
    extern __shared__ __attribute__((aligned(16))) char lds_all[];
    const unsigned lane = threadIdx.x;
    const uint64_t n = a.val.n_blocks;
    const uint64_t first = (uint64_t)blockIdx.x * a.run;
    if (first >= n) return;
    const uint64_t end = n - first < a.run ? n : first + a.run;
    BlockAggregate* table = reinterpret_cast<BlockAggregate*>(lds_all + G::BLOCK_BYTES);
    if constexpr (TIER == AGGW_LDS) {
        for (unsigned g = lane; g < a.n_slots; g += 64u) {                  // only the window's slots
            u32x4* s = reinterpret_cast<u32x4*>(table + g);
            s[0] = u32x4{0u, 0u, 0u, 0u};                                   // count, sum
            s[1] = u32x4{~0u, ~0u, 0u, 0u};                                 // min, max
        }
        wave_lds_fence();
    }
    uint64_t ins = 0, out = 0;
    WindowBlockLoads<T> cur = aggregate_by_window_issue<T>(a, first, lane);
    for (uint64_t blk = first; blk < end; ++blk) {                          // wave-uniform loop
        const uint64_t ahead = blk + 1 < end ? blk + 1 : blk;               // the last block asks for itself again: straight-line code
        const WindowBlockLoads<T> nxt = aggregate_by_window_issue<T>(a, ahead, lane);
        aggregate_by_window_block<T, TIER>(a, blk, cur, lds_all, table, lane, ins, out);
        cur = nxt;
    }
    if constexpr (TIER == AGGW_LDS) {
        wave_lds_fence();
        for (unsigned g = lane; g < a.n_slots; g += 64u) {                  // as group_table_flush: only what this wavefront has updated
            const BlockAggregate s = table[g];
            if (s.count != 0ull) window_arrays_update(a, g, s.count, s.sum, s.min, s.max);
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
hipError_t launch_aggregate_by_window(const AggregateByWindowArgs& a, int waves, hipStream_t s)
{
    return launch_group_runs<k_unfor_aggregate_by_window<T, TIER>, aggregate_by_window_lds<T, TIER>()>(a, a.val.n_blocks, a.val.bpw, waves, s);
}

typedef hipError_t (*aggregate_by_window_launch_t)(const AggregateByWindowArgs&, int waves, hipStream_t);
template <typename T> aggregate_by_window_launch_t aggregate_by_window_launcher(int tier);

}  // namespace fl
