// fl_aggregate_by_lookup.hpp -- unfor_aggregate_by_lookup: COUNT / SUM / MIN / MAX of a FoR-packed VALUE column grouped by a u8
// attribute of a dimension table, fetched through a FoR-packed KEY column of the SAME element type and block count inside a dense window
// of the key domain, over the rows a selection mask keeps (SUM(revenue) GROUP BY n_name through l_suppkey): unfor_lookup_u8 and
// unfor_aggregate_by in ONE pass, with no per-row output -- no code column, no hit mask.  EXTENSION, defined as a
// composition of reference functions; all key arithmetic mod 2^T:
//     result[g] = identity {0, 0, UINT64_MAX, 0}                                          for g = 0 .. 255 (k_aggregate_by_init)
//     for every block b, every i with bit i of block b of `mask` set (mask == nullptr: every i):
//         val = unfor_pack::<W_b >(value block b, references[b * ref_stride])[i]                  zero-extended      (ffor.rs:38-50)
//         key = unfor_pack::<KW_b>(key block b, key_references[b * key_ref_stride])[i]
//         j   = (key - key_lo) mod 2^T
//         hit = j < n_slots and (present == nullptr or bit j of present)
//         hit:  g = table[j];  result[g] = combine(result[g], {1, val, val, val});  hits += 1
//         else: misses += 1
//     stats[0] += hits;  stats[1] += misses
// which is, bit for bit in result and stats, unfor_lookup_u8 into a temporary with its hit mask followed by unfor_aggregate_by with the
// temporary as the full-width u8 key column and mask = the hits.  Integer add, min and max commute: the result is bitwise reproducible.
// The window is unfor_set_build's (fl_set_decide.hpp), and with c = (key reference - key_lo) the f + c of the compare kernels is j.
// A run-walking kernel (fl_block_run.hpp: the run, the look-ahead, the wave-private table of 256 BlockAggregate and its flush into
// result[256], behind k_aggregate_by_init on the same stream, the stats tail, the fetch of two columns through ONE image).  Per block,
// through the steps of fl_for_block.hpp: both columns' preconditions are checked; the route comes from fl_aggregate_by_lookup_map.hpp
// (aggregate_by_lookup_route): a failed check and an empty mask read nothing, a key block outside the window reads neither column and no
// table byte, a width-0 key block inside it is one wave-uniform table read (and at most one `present` bit) and then unfor_aggregate's
// block folded into group table[c] by lane 0.  Every other block fetches both columns under ONE wait, as unfor_aggregate_by_window
// does -- the key rows into the wavefront's image, the value rows into staging registers.  The lane
// keeps its 16 slots j = f + c in registers, issues its 16 code gathers and then its 16 `present` words (when a bitmap is given) before
// it looks at the first, and meanwhile the staged value rows overwrite the dead image and are funnelled in the same lane map.  A row the
// mask drops or whose key lies outside the window is given the offset LOOKUP_PAST, which reads 0 and touches no memory; its gathered 0
// is NEVER used as a group (0 is a valid code): only a row whose `want` bit survives updates the table.  No key area.
// ONE table tier: the cached, bounded gather of unfor_lookup's memory tier (lookup_fetch<uint8_t, LOOKUP_MEM>).  There is no LDS copy of
// the dimension table: unfor_lookup measured its LDS tier slower than its memory tier at the boundary (0.793 ms at 8192 slots against
// 0.521 ms at 8193) and no faster at 25 slots, and here the LDS already holds the group table.  `present` is gathered through its own
// bounded descriptor with the cached policy.
// Hits and misses are counted per lane (folded with wave_sum_u64, fl_block_run.hpp).  A block that fails the mixed-width device checks of either column raises its FL_DEVERR_* bits and
// contributes nothing.  LDS is wave-local (in-order per wave): no s_barrier.  Every global store or atomic is a vector instruction.
// Out of scope: a value type different from the key type; payloads wider than u8 or more than 256 groups (unfor_aggregate_by_window
// after a T-payload lookup serves those); several tables or an a op b expression per launch; an LDS copy of the dimension table; sparse
// or hashed keys; Delta columns; the host tier; tables of 2^31 bytes or more.
#pragma once
#include "fl_aggregate_by_lookup_map.hpp"
#include "fl_aggregate_by_window.hpp"
#include "fl_lookup.hpp"
#include "fl_set_build.hpp"

namespace fl {

// WidthsArgs::refs and ::unpacked stay nullptr in both columns: the references are loaded with the blocks' metadata
struct AggregateByLookupArgs {
    WidthsArgs val, key;           // the same n_blocks, the same err_flag
    const void* val_refs;          // references[b * val.ref_stride]
    const void* key_refs;          // key_references[b * key.ref_stride]
    const uint32_t* mask;          // [n_blocks][32]; nullptr = every row is kept (no mask is read)
    const void* table;             // uint8_t[n_slots]; never read when n_slots == 0
    const uint32_t* present;       // ceil(n_slots / 32) words; nullptr = every slot is present
    BlockAggregate* result;        // [256]
    uint64_t* stats;               // {hits, misses}; nullptr = not counted
    uint64_t cmp_a, cmp_s;         // the window as a ForPredicate: key_lo, n_slots - 1
    unsigned cmp_none;             // n_slots == 0
    unsigned table_bytes;          // n_slots < 2^31: the table descriptor's size
    unsigned present_bytes;        // 4 * ceil(n_slots / 32): the bitmap descriptor's size
    uint64_t run;                  // blocks of a wavefront's run; filled by the launcher
};

template <typename T> constexpr unsigned aggregate_by_lookup_lds() { return aggregate_by_lookup_wave_lds(WaveBlock<T>::BLOCK_BYTES); }

// one block whose loads were issued by aggregate_by_window_issue.  lds: [image | group table]; hit / miss: the lane's counters
template <typename T>
__device__ __forceinline__ void aggregate_by_lookup_block(const AggregateByLookupArgs& a, uint64_t blk, const WindowBlockLoads<T>& p, char* lds,
                                                          BlockAggregate* table, const __amdgpu_buffer_rsrc_t& ts, const __amdgpu_buffer_rsrc_t& ps,
                                                          unsigned lane, uint64_t& hit, uint64_t& miss)
{
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    constexpr int N = Elem<T>::PER_CELL, GROUPS = G::GROUPS;
    static_assert(M::GROUPS == (unsigned)GROUPS && M::N == (unsigned)N, "fl_select_map.hpp follows fl_widths.hpp's lane map");
    static_assert(GROUPS * N == 16, "16 elements per lane whatever the type");
    const BlockMeta mv = settle_block_loads<T>(a.val, blk, p.v);
    const BlockMeta mk = settle_block_loads<T>(a.key, blk, p.k);
    uint32_t any = 0;
    static_for<GROUPS>([&](auto K) { any |= p.slice[decltype(K)::value]; });
    const bool empty = __builtin_amdgcn_ballot_w64(any != 0u) == 0ull;
    const uint32_t err = mv.err | mk.err;
    if (err) raise_device_error(a.val.err_flag, err, lane);
    uint64_t c;
    const AggregateByLookupRoute route =
        aggregate_by_lookup_route(G::TB, ForPredicate{a.cmp_a, a.cmp_s, a.cmp_none != 0u}, empty, err == 0u, mk.r, mk.w, c);
    if (route == AGGL_SKIP || route == AGGL_NOTHING) return;
    const uint32_t kept = aggregate_lane_of<T>(p.slice).count;              // the lane's kept rows
    if (route == AGGL_MISSING) {
        miss += kept;
        return;
    }
    const T r = (T)mv.r;
    if (route == AGGL_ONE_GROUP) {                                          // width 0 inside the window: slot c, c wave-uniform
        uint32_t word = ~0u;
        if (a.present) word = (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_amdgcn_raw_buffer_load_b32(ps, (uint32_t)(c >> 5) << 2, 0, 0));
        if (((word >> (c & 31u)) & 1u) == 0u) {                             // the slot is absent: as a block outside the window
            miss += kept;
            return;
        }
        // one address for the wavefront; unfor_aggregate's block, folded into group table[c]
        const unsigned code = (unsigned)__builtin_amdgcn_readfirstlane((int)lookup_fetch<uint8_t, LOOKUP_MEM>(ts, nullptr, (uint32_t)c, true)) & 0xffu;
        BlockAggregate g;
        if (mv.w == 0u) {
            g = aggregate_constant_block(aggregate_wave_count(kept), (uint64_t)r);
        } else {
            fill_block_image<T>(a.val, blk, mv.off, mv.w, lds, lane);
            g = aggregate_lds_image<T>(mv.w, lds, lane, r, p.slice);
            wave_lds_fence();                                               // the image is reused by the wavefront's next block
        }
        if (lane == 0u) group_table_update(table, code, g.count, g.sum, g.min, g.max);
        hit += kept;
        return;
    }
    // both columns under one wait: wave-uniform descriptors over exactly each block's bytes (a width-0 value block: none); the key rows
    // (1 <= key width <= T) by LDS-DMA into the image, the value rows into staging registers
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.key.packed) + mk.off, 0, 128u * mk.w, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.val.packed) + mv.off, 0, 128u * mv.w, 0x00020000);
    const StagedRows<T> pk = request_image_and_staged<T>(krs, mk.w, vrs, mv.w, lds, lane);
    wait_lds_dma();
    wave_lds_fence();
    // the key block: the lane's 16 slots j = f + c into registers; bit i of `want`: element i is kept and inside the window
    const Cell<T> cc = Cell<T>::splat((T)c);
    const T s = (T)a.cmp_s;
    uint32_t at[16];
    uint32_t want = 0;
    for_each_funnelled_cell<T>(mk.w, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) {
        const Cell<T> j = cell.add(cc);                                     // (f + c) mod 2^T per element: the slot
        const uint32_t sl = p.slice[decltype(K)::value];
        static_for<N>([&](auto E) {
            constexpr int i = decltype(K)::value * N + decltype(E)::value;
            const T x = (T)cell_get<T>(j, decltype(E)::value);
            const bool in = ((sl >> decltype(E)::value) & 1u) != 0u && x <= s;
            at[i] = (uint32_t)x;                                            // a slot inside the window is < 2^31
            want |= (in ? 1u : 0u) << i;
        });
    });
    // the lane's 16 code gathers, then its 16 bitmap words: all requested before the first is looked at
    uint8_t code[16];
    uint32_t word[16];
    static_for<16>([&](auto I) {
        constexpr int i = decltype(I)::value;
        code[i] = lookup_fetch<uint8_t, LOOKUP_MEM>(ts, nullptr, at[i], ((want >> i) & 1u) != 0u);
    });
    if (a.present) {
        static_for<16>([&](auto I) {
            constexpr int i = decltype(I)::value;
            word[i] = __builtin_amdgcn_raw_buffer_load_b32(ps, ((want >> i) & 1u) != 0u ? (at[i] >> 5) << 2 : LOOKUP_PAST, 0, 0);
        });
    }
    staged_to_image<T>(pk, mv.w, lds, lane);
    if (a.present) {
        static_for<16>([&](auto I) {
            constexpr int i = decltype(I)::value;
            want &= ~((((word[i] >> (at[i] & 31u)) & 1u) ^ 1u) << i);       // a clear bit: no hit (a word past the bitmap reads 0)
        });
    }
    // the value block through the same lane map (width 0: every field is 0, the value is the reference); only a hit reaches the table
    const Cell<T> rc = Cell<T>::splat(r);
    for_each_funnelled_cell<T>(mv.w, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) {
        constexpr int k = decltype(K)::value;
        const Cell<T> v = cell.add(rc);                                     // ffor.rs:46-48
        static_for<N>([&](auto E) {
            constexpr int e = decltype(E)::value;
            constexpr int i = k * N + e;
            if (((want >> i) & 1u) != 0u) {
                const uint64_t x = (uint64_t)cell_get<T>(v, e);
                group_table_update(table, (unsigned)code[i], 1ull, x, x, x);
            }
        });
    });
    const uint32_t n_hit = (uint32_t)__builtin_popcount(want);
    hit += n_hit;
    miss += kept - n_hit;
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

// Workgroup (= wavefront) g owns blocks [g * run, (g + 1) * run) of the column; one that owns none returns before it touches LDS.
template <typename T>
__global__ __launch_bounds__(64) void k_unfor_aggregate_by_lookup(AggregateByLookupArgs a)
{
    using G = WaveBlock<T>;
    extern __shared__ __attribute__((aligned(16))) char lds_all[];
    const unsigned lane = threadIdx.x;
    const uint64_t n = a.val.n_blocks;
    const uint64_t first = (uint64_t)blockIdx.x * a.run;
    if (first >= n) return;
    const uint64_t end = n - first < a.run ? n : first + a.run;
    BlockAggregate* table = reinterpret_cast<BlockAggregate*>(lds_all + G::BLOCK_BYTES);
    const __amdgpu_buffer_rsrc_t ts = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.table), 0, a.table_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ps = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(a.present), 0, a.present_bytes, 0x00020000);
    WindowBlockLoads<T> cur = aggregate_by_window_issue<T>(a, first, lane);   // in flight while the group table is initialised
    for (unsigned g = lane; g < AGGREGATE_BY_LOOKUP_GROUPS; g += 64u) {
        u32x4* s = reinterpret_cast<u32x4*>(table + g);
        s[0] = u32x4{0u, 0u, 0u, 0u};                                       // count, sum
        s[1] = u32x4{~0u, ~0u, 0u, 0u};                                     // min, max
    }
    wave_lds_fence();
    uint64_t hit = 0, miss = 0;
    for (uint64_t blk = first; blk < end; ++blk) {                          // wave-uniform loop
        const uint64_t ahead = blk + 1 < end ? blk + 1 : blk;               // the last block asks for itself again: straight-line code
        const WindowBlockLoads<T> nxt = aggregate_by_window_issue<T>(a, ahead, lane);
        aggregate_by_lookup_block<T>(a, blk, cur, lds_all, table, ts, ps, lane, hit, miss);
        cur = nxt;
    }
    group_table_flush(table, AGGREGATE_BY_LOOKUP_GROUPS, a.result, lane);
    if (a.stats) {
        hit = wave_sum_u64(hit);
        miss = wave_sum_u64(miss);
        if (lane == 0u && hit != 0ull) __hip_atomic_fetch_add(a.stats, hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0u && miss != 0ull) __hip_atomic_fetch_add(a.stats + 1, miss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <typename T>
hipError_t launch_aggregate_by_lookup(const AggregateByLookupArgs& a, int waves, hipStream_t s)
{
    return launch_group_runs<k_unfor_aggregate_by_lookup<T>, aggregate_by_lookup_lds<T>()>(a, a.val.n_blocks, a.val.bpw, waves, s);
}

typedef hipError_t (*aggregate_by_lookup_launch_t)(const AggregateByLookupArgs&, int waves, hipStream_t);
template <typename T> aggregate_by_lookup_launch_t aggregate_by_lookup_launcher();

}  // namespace fl
