// fl_aggregate_by_columns.hpp -- unfor_aggregate_by_columns: COUNT / SUM / MIN / MAX of `a o b` between two FoR-packed VALUE columns of one
// element type (u8 / u16 / u32 / u64) grouped by a FoR-packed u8 KEY column of the same block count, over the rows a selection mask
// keeps (no mask: every row) -- SELECT k, SUM(price * discount) WHERE <mask> GROUP BY k, with none of the three columns materialised.
// EXTENSION, the join of unfor_aggregate_by and unfor_aggregate_columns, defined as a composition of reference functions:
//     va  = unfor_pack::<WA_b>(a block b, a_references[b * a_ref_stride])[i]       vb likewise from column b           (ffor.rs:38-50)
//     key = unfor_pack::<KW_b>(key block b, key_references[b * key_ref_stride])[i]                           (u8, wrapping add)
//     x   = expr_apply(expr, zext64(va), zext64(vb))                      (fl_expr_map.hpp: MUL, ADD, SUB = a - b, mod 2^64)
//     result[g] = combine over all (b, i) with mask bit (b, i) set and key == g of {1, x, x, x}                (g = 0 .. 255)
// A run-walking kernel (fl_block_run.hpp: the run, the look-ahead, the table and its flush); the LDS layout, the key area and the init
// launch in front are fl_aggregate_by.hpp's, the fetch of two value columns through ONE image is fl_aggregate_columns.hpp's.  Per block:
//   * the three preconditions are checked: a block that fails any raises its bits and contributes nothing, none of its columns is read;
//   * the route comes from fl_aggregate_by_columns_map.hpp: an EMPTY mask reads nothing; key width 0 is unfor_aggregate_columns' block
//     with its own constant and decode routes (expr_constant_block, expr_lds_image: the copies that kernel runs), its one BlockAggregate
//     folded into the slot of the key reference by lane 0, no key byte read;
//   * a block that decodes fetches under ONE wait: the key rows by LDS-DMA into the key area (key width >= 1 only), column a's rows by
//     LDS-DMA into the image, column b's rows into staging registers -- only columns of width >= 1 request anything, descriptors over
//     exactly each block's 128 * w bytes.  The key block is decoded first and its 1024 keys stored in index order; column a is funnelled
//     into registers; column b's staged rows overwrite the dead image and are funnelled in the same lane map; every kept element
//     computes x in 64 bits (expr_apply on the zero-extended values: the LDS atomics dominate, ExprLane's narrow accumulators would buy
//     nothing) and updates its key's slot.  The fetch is ONE path for the keyed and the one-key block (wave-uniform branches).
// LDS per wavefront is aggregate_by_wave_lds: the residency of unfor_aggregate_by for every type.  No scratch memory.
// LDS is wave-local (in-order per wave): no s_barrier.  Every global store or atomic is a vector instruction.
#pragma once
#include "fl_aggregate_by.hpp"
#include "fl_aggregate_by_columns_map.hpp"
#include "fl_aggregate_columns.hpp"

namespace fl {

// WidthsArgs::refs and ::unpacked stay nullptr in the three columns: the references are loaded with the blocks' metadata
struct AggregateByColumnsArgs {
    WidthsArgs a, b, key;          // the same n_blocks, the same err_flag
    const void* a_refs;            // a_references[b * a.ref_stride]
    const void* b_refs;            // b_references[b * b.ref_stride]
    const void* key_refs;          // key_references[b * key.ref_stride]
    const uint32_t* mask;          // [n_blocks][32]; nullptr = every row is kept (no mask is read)
    BlockAggregate* result;        // [256]
    uint64_t run;                  // blocks of a wavefront's run; filled by the launcher
    unsigned expr;                 // EXPR_MUL / EXPR_ADD / EXPR_SUB, validated by the host
};

// a block's loads, issued and possibly still in flight: aggregate_by_issue with a third column
template <typename T> struct GroupColumnsBlockLoads {
    BlockLoads<T> a, b;
    BlockLoads<uint8_t> k;
    uint32_t slice[SelectMap<sizeof(T)>::GROUPS];
};
template <typename T>
__device__ __forceinline__ GroupColumnsBlockLoads<T> aggregate_by_columns_issue(const AggregateByColumnsArgs& a, uint64_t blk, unsigned lane)
{
    GroupColumnsBlockLoads<T> p;
    p.a = issue_block_loads<T>(a.a, a.a_refs, blk);
    p.b = issue_block_loads<T>(a.b, a.b_refs, blk);
    p.k = issue_block_loads<uint8_t>(a.key, a.key_refs, blk);
    block_mask_slices<T>(a.mask, blk, lane, p.slice);
    return p;
}

// Column a's values (reference added) against the LDS image of column b's wb rows (wb = 0: every field is 0, the value is the
// reference): every kept element's a OP b into the slot of its key, read from the key area
template <typename T, int OP>
__device__ __forceinline__ void group_expr_lds_image(const Cell<T> (&va)[WaveBlock<T>::GROUPS], unsigned wb, const char* lds, const char* key_lds,
                                                     BlockAggregate* table, unsigned lane, T rb, const uint32_t (&slice)[SelectMap<sizeof(T)>::GROUPS])
{
    using M = SelectMap<sizeof(T)>;
    const Cell<T> cb = Cell<T>::splat(rb);
    for_each_funnelled_cell<T>(wb, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) {
        constexpr unsigned k = decltype(K)::value;
        const Cell<T> vb = cell.add(cb);                                    // ffor.rs:46-48, in T
        const uint32_t sl = slice[k];
        uint32_t kw[4];
        cell_keys<T>(key_lds, k, lane, kw);
        static_for<(int)M::N>([&](auto E) {
            constexpr unsigned e = decltype(E)::value;
            if ((sl >> e) & 1u) {
                const uint64_t x = expr_apply(OP, (uint64_t)cell_get<T>(va[k], (int)e), (uint64_t)cell_get<T>(vb, (int)e));
                group_table_update(table, (kw[e / 4u] >> (8u * (e % 4u))) & 0xffu, 1ull, x, x, x);
            }
        });
    });
}

// the meeting of the two value columns under OP: a keyed block updates every kept element's slot; a block of ONE key is
// unfor_aggregate_columns' block (expr_lds_image: masked accumulate and butterfly) and lane 0 folds its aggregate into slot `one_key`
template <typename T, int OP>
__device__ __forceinline__ void group_expr_meet(bool keyed, unsigned one_key, const Cell<T> (&va)[WaveBlock<T>::GROUPS], unsigned wb, const char* lds,
                                                const char* key_lds, BlockAggregate* table, unsigned lane, T rb,
                                                const uint32_t (&slice)[SelectMap<sizeof(T)>::GROUPS])
{
    if (keyed) {
        group_expr_lds_image<T, OP>(va, wb, lds, key_lds, table, lane, rb, slice);
        return;
    }
    const BlockAggregate g = expr_lds_image<T, OP>(va, wb, lds, lane, rb, slice);
    if (lane == 0u) group_table_update(table, one_key, g.count, g.sum, g.min, g.max);
}

// one block whose loads were issued by aggregate_by_columns_issue.  lds: [value image | key area | table]
template <typename T>
__device__ __forceinline__ void aggregate_by_columns_block(const AggregateByColumnsArgs& a, uint64_t blk, const GroupColumnsBlockLoads<T>& p, char* lds,
                                                           unsigned lane)
{
    using G = WaveBlock<T>;
    char* key_lds = lds + G::BLOCK_BYTES;
    BlockAggregate* table = reinterpret_cast<BlockAggregate*>(key_lds + AGGREGATE_BY_KEY_BYTES);
    const BlockMeta ma = settle_block_loads<T>(a.a, blk, p.a);
    const BlockMeta mb = settle_block_loads<T>(a.b, blk, p.b);
    const BlockMeta mk = settle_block_loads<uint8_t>(a.key, blk, p.k);
    uint32_t any = 0;
    static_for<(int)SelectMap<sizeof(T)>::GROUPS>([&](auto K) { any |= p.slice[decltype(K)::value]; });
    const bool empty = __builtin_amdgcn_ballot_w64(any != 0u) == 0ull;
    const uint32_t err = ma.err | mb.err | mk.err;
    if (err) raise_device_error(a.a.err_flag, err, lane);
    const AggregateByColumnsRoute route = aggregate_by_columns_route(empty, err == 0u, mk.w, ma.w, mb.w);
    if (route.by == AGGBY_SKIP) return;
    const bool keyed = route.by == AGGBY_DECODE;                            // else ONE_KEY: every kept row carries the key reference
    const unsigned one_key = (unsigned)mk.r & 0xffu;
    if (!keyed && route.expr <= EXPR_CONSTANT) {                            // no packed load at all: count x (ra o rb), the count from the mask bits
        const BlockAggregate g = expr_constant_block((int)a.expr, aggregate_wave_count(aggregate_lane_of<T>(p.slice).count), ma.r, mb.r);
        if (lane == 0u) group_table_update(table, one_key, g.count, g.sum, g.min, g.max);
        return;
    }
    // the columns' rows, one wait; wave-uniform descriptors over exactly each block's 128 * w bytes (a width-0 column: none, nothing is
    // requested of it; ONE_KEY: no key byte)
    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.a.packed) + ma.off, 0, 128u * ma.w, 0x00020000);
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.b.packed) + mb.off, 0, 128u * mb.w, 0x00020000);
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.key.packed) + mk.off, 0, 128u * mk.w, 0x00020000);
    if (keyed) dma_1k_to_lds<RD_DMA_NT, 0>(krs, key_lds, lane);             // 1 <= key width <= 8: one KiB, bytes past the block arrive as 0
    static_for<G::GROUPS>([&](auto Gi) {
        constexpr int g = decltype(Gi)::value;
        if (8u * g < ma.w) dma_1k_to_lds<RD_DMA_NT, g * 1024>(ars, lds, lane);
    });
    u32x4 pk[G::GROUPS];
    static_for<G::GROUPS>([&](auto Gi) {
        constexpr int g = decltype(Gi)::value;
        if (8u * g < mb.w) pk[g] = __builtin_amdgcn_raw_buffer_load_b128(brs, lane * 16u + g * 1024u, 0, 2);   // non-temporal, as the DMA
    });
    wait_lds_dma();
    wave_lds_fence();
    if (keyed) decode_keys_to_area(mk.w, (uint8_t)mk.r, key_lds, lane);     // the key block first
    // column a: the lane's 16 values into registers (W = 0: every field is 0, the value is the reference)
    Cell<T> va[G::GROUPS];
    const Cell<T> ra = Cell<T>::splat((T)ma.r);
    for_each_funnelled_cell<T>(ma.w, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) { va[decltype(K)::value] = cell.add(ra); });
    wave_lds_fence();                                                       // every lane holds column a's values: the image is dead
    static_for<G::GROUPS>([&](auto Gi) {
        constexpr int g = decltype(Gi)::value;
        if (8u * g < mb.w) *reinterpret_cast<u32x4*>(lds + lane * 16u + g * 1024u) = pk[g];
    });
    wave_lds_fence();                                                       // column b's image and the key area are written
    const T rb = (T)mb.r;                                                   // the op is wave-uniform
    if (a.expr == EXPR_MUL) group_expr_meet<T, EXPR_MUL>(keyed, one_key, va, mb.w, lds, key_lds, table, lane, rb, p.slice);
    else if (a.expr == EXPR_ADD) group_expr_meet<T, EXPR_ADD>(keyed, one_key, va, mb.w, lds, key_lds, table, lane, rb, p.slice);
    else group_expr_meet<T, EXPR_SUB>(keyed, one_key, va, mb.w, lds, key_lds, table, lane, rb, p.slice);
    wave_lds_fence();                                                       // image and key area are reused by the wavefront's next block
}

// Workgroup (= wavefront) g owns blocks [g * run, (g + 1) * run) of the columns; one that owns none returns at once.
template <typename T>
__global__ __launch_bounds__(64) void k_unfor_aggregate_by_columns(AggregateByColumnsArgs a)
{
    using G = WaveBlock<T>;
    extern __shared__ __attribute__((aligned(16))) char lds_all[];
    const unsigned lane = threadIdx.x;
    const uint64_t n = a.a.n_blocks;
    const uint64_t first = (uint64_t)blockIdx.x * a.run;
    if (first >= n) return;
    const uint64_t end = n - first < a.run ? n : first + a.run;
    BlockAggregate* table = reinterpret_cast<BlockAggregate*>(lds_all + G::BLOCK_BYTES + AGGREGATE_BY_KEY_BYTES);
    for (unsigned g = lane; g < AGGREGATE_BY_GROUPS; g += 64u) {            // as k_unfor_aggregate_by
        u32x4* s = reinterpret_cast<u32x4*>(table + g);
        s[0] = u32x4{0u, 0u, 0u, 0u};                                       // count, sum
        s[1] = u32x4{~0u, ~0u, 0u, 0u};                                     // min, max
    }
    wave_lds_fence();
    GroupColumnsBlockLoads<T> cur = aggregate_by_columns_issue<T>(a, first, lane);
    for (uint64_t blk = first; blk < end; ++blk) {                          // wave-uniform loop
        const uint64_t ahead = blk + 1 < end ? blk + 1 : blk;               // the last block asks for itself again: straight-line code
        const GroupColumnsBlockLoads<T> nxt = aggregate_by_columns_issue<T>(a, ahead, lane);
        aggregate_by_columns_block<T>(a, blk, cur, lds_all, lane);
        cur = nxt;
    }
    group_table_flush(table, AGGREGATE_BY_GROUPS, a.result, lane);
}

// the launch of unfor_aggregate_by (launch_group_runs): the same grid, the same LDS request, the same run rule
template <typename T>
hipError_t launch_aggregate_by_columns(const AggregateByColumnsArgs& a, int waves, hipStream_t s)
{
    return launch_group_runs<k_unfor_aggregate_by_columns<T>, aggregate_by_lds<T>()>(a, a.a.n_blocks, a.a.bpw, waves, s);
}

typedef hipError_t (*aggregate_by_columns_launch_t)(const AggregateByColumnsArgs&, int waves, hipStream_t);
template <typename T> aggregate_by_columns_launch_t aggregate_by_columns_launcher();

}  // namespace fl
