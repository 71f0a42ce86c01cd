// fl_aggregate_columns.hpp -- unfor_aggregate_columns: COUNT / SUM / MIN / MAX per block of `a o b` between two FoR-packed columns of the
// same element type and block count, both uniform width (possibly different widths) or both mixed width, over the rows a selection mask
// keeps (no mask: every row) -- SELECT SUM(price * discount), SUM(bid - ask), MAX(a + b), a dot product, with neither column materialised.
// EXTENSION, defined as a composition of reference functions:
//     va = unfor_pack::<WA_b>(a block b, a_references[b * a_ref_stride])[i]       vb likewise from column b        (ffor.rs:38-50)
//     x[b][i] = (zext64(va) o zext64(vb)) mod 2^64          o: EXPR_MUL, EXPR_ADD, EXPR_SUB (a - b)       (fl_expr_map.hpp: expr_apply)
//     agg_b   = { count, sum x (wrapping), min x, max x } over the i whose mask bit is set      (nothing kept: {0, 0, UINT64_MAX, 0})
// The values are widened BEFORE the operation: u8 / u16 / u32 products and sums are exact, u64 wraps; a difference below zero is its
// two's-complement bit pattern, so SUM stays right mod 2^64, and MIN / MAX compare the patterns as UNSIGNED numbers.  The slots, the
// mask and the reduction over the slots (fl_scan.hpp: launch_aggregate_reduce) are unfor_aggregate's.
// One wavefront per block in the launch shape of unfor_pack_widths, through the steps of fl_for_block.hpp, the fetch of
// fl_for_compare_columns.hpp and the slot of fl_aggregate.hpp:
//   * both columns' width, offset and reference AND the lane's mask slices arrive together (independent vector loads, one wait); both
//     columns' preconditions are checked: a block that fails either raises its bits, reads neither column and its slot receives the
//     IDENTITY -- the slot feeds a reduction, so a skipped block must not leave stale memory in it;
//   * a block whose mask is EMPTY writes the identity, one whose two widths are both 0 writes count x (ra o rb), the count from the
//     mask bits alone: neither issues a packed load (fl_expr_map.hpp: expr_route, expr_constant_block);
//   * otherwise only the columns of width >= 1 are fetched (a width-0 side requests nothing and decodes to its reference), both under
//     ONE wait: column a's rows by LDS-DMA into the wavefront's image, column b's rows into staging registers.  ONE image serves both
//     columns, which keeps the launch shape, the LDS request and the residency of unfor_aggregate for every type: lane (i, c) funnels
//     its cell of every 1-KiB group of column a, adds the reference in T and keeps the 16 values in registers (4 / 8 / 16 / 32 VGPRs
//     for u8 / u16 / u32 / u64); the staged rows of column b then overwrite the dead image and are funnelled in the same lane map;
//   * per element: the second reference add in T, both values widened, `o`, and the masked accumulate (ExprLane: exact per type and
//     op); ONE butterfly over the 64 lanes (__shfl_xor) reduces count, sum, min and max together; the count is the popcount of the
//     lane's mask bits, never taken from the data path;
//   * lanes 0 and 1 store the slot's two 16-byte halves (store_block_aggregate).
// Every launch shape for_each_block_of_wave hands out is served block by block through the wavefront's first image; a
// several-blocks-in-flight form for the narrow types is an open end.
// Out of scope: signed (sign-extending) columns, columns of different element types, Delta columns, grouping, the host tier.
// LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_aggregate.hpp"
#include "fl_expr_map.hpp"

namespace fl {

// The AggregateArgs base is column a (it carries the launch shape, the tile map, the mask and the slots), agg_refs its references.
// Both columns have the same n_blocks and the same err_flag.
struct AggregateColumnsArgs : AggregateArgs {
    WidthsArgs b;              // column b
    const void* b_refs;        // b_references[blk * b.ref_stride]
    unsigned expr;             // EXPR_MUL / EXPR_ADD / EXPR_SUB, validated by the host
};

// What a lane holds of its 16 elements of `a OP b`, and in which widths.  Every choice is EXACT: nothing can overflow before the
// block's aggregate is widened to the slot's 64 bits.
//   u8:   x = a o b in 32 bits: a product < 2^16, a sum < 2^9, a difference in (-2^8, 2^8) as its 32-bit pattern.  A block's 1024 of
//         them sum to a magnitude < 2^26: the lane's and the butterfly's sums take 32 bits (signed, wrapping, for SUB).
//   u16:  x in 32 bits: a product <= (2^16 - 1)^2 < 2^32, a sum < 2^17, a difference in (-2^16, 2^16).  Sixteen products already pass
//         2^32, so MUL sums in 64 bits; ADD and SUB sum to a magnitude < 2^27 per block: 32 bits.
//   u32 / u64:  x, sum, min and max in 64 bits -- expr_apply itself: u32 is exact (a product < 2^64, a sum < 2^33), u64 wraps as the
//         definition does.
// SUB of the narrow types: the 32-bit results are SIGN-extended at the end (SEXT).  That is the 64-bit pattern of the same number, and
// sign extension keeps the unsigned order of the patterns (every negative one lies above every non-negative one at either width), so
// the minimum and maximum chosen in 32 bits are the ones the definition chooses in 64.
template <typename T, int OP> struct ExprLane {
    static constexpr bool NARROW = sizeof(T) <= 2;
    static constexpr bool SEXT = NARROW && OP == EXPR_SUB;
    using x_t = std::conditional_t<NARROW, uint32_t, uint64_t>;
    using sum_t = std::conditional_t<sizeof(T) == 1 || (sizeof(T) == 2 && OP != EXPR_MUL), uint32_t, uint64_t>;
    uint32_t count;
    sum_t sum;
    x_t min, max;
    __device__ __forceinline__ static uint64_t widen(uint32_t v) { return SEXT ? (uint64_t)(int64_t)(int32_t)v : (uint64_t)v; }
    __device__ __forceinline__ static uint64_t widen(uint64_t v) { return v; }
};

// the 64 lanes' partial aggregates -> the block's, in every lane: one butterfly, the four chains independent of each other.  Only
// reached with count > 0: the minimum is then a value, not the accumulator's all-ones start.
template <typename T, int OP> __device__ __forceinline__ BlockAggregate expr_wave_reduce(ExprLane<T, OP> l)
{
    using L = ExprLane<T, OP>;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t c = __shfl_xor(l.count, d, 64);
        const typename L::sum_t s = __shfl_xor(l.sum, d, 64);
        const typename L::x_t lo = __shfl_xor(l.min, d, 64), hi = __shfl_xor(l.max, d, 64);
        l.count += c;
        l.sum += s;
        l.min = lo < l.min ? lo : l.min;
        l.max = hi > l.max ? hi : l.max;
    }
    return BlockAggregate{l.count, L::widen(l.sum), L::widen(l.min), L::widen(l.max)};
}

// Column a's kept values (reference added) against the LDS image of column b's wb rows (wb = 0: every field is 0, the value is the
// reference) -> the block's aggregate of a OP b over the lane's slice bits, in every lane
template <typename T, int OP>
__device__ __forceinline__ BlockAggregate expr_lds_image(const Cell<T> (&va)[WaveBlock<T>::GROUPS], unsigned wb, const char* lds, unsigned lane, T rb,
                                                         const uint32_t (&slice)[SelectMap<sizeof(T)>::GROUPS])
{
    using M = SelectMap<sizeof(T)>;
    using L = ExprLane<T, OP>;
    using x_t = typename L::x_t;
    using sum_t = typename L::sum_t;
    static_assert(M::GROUPS == (unsigned)WaveBlock<T>::GROUPS && M::N == (unsigned)Elem<T>::PER_CELL, "fl_select_map.hpp follows fl_widths.hpp's lane map");
    L l{aggregate_lane_of<T>(slice).count, (sum_t)0, ~(x_t)0, (x_t)0};
    const Cell<T> cb = Cell<T>::splat(rb);
    for_each_funnelled_cell<T>(wb, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) {
        constexpr int k = decltype(K)::value;
        const Cell<T> vb = cell.add(cb);                                    // ffor.rs:46-48, in T
        const uint32_t sl = slice[k];
        static_for<(int)M::N>([&](auto E) {
            constexpr int e = decltype(E)::value;
            const x_t p = (x_t)cell_get<T>(va[k], e), q = (x_t)cell_get<T>(vb, e);   // zero-extended
            const x_t x = OP == EXPR_MUL ? p * q : OP == EXPR_ADD ? p + q : p - q;  // expr_apply, at the width ExprLane proves exact
            const bool on = ((sl >> e) & 1u) != 0u;
            l.sum += on ? (sum_t)x : (sum_t)0;                              // (a narrow SUB: the low 32 bits of the sign-extended sum)
            l.min = on && x < l.min ? x : l.min;
            l.max = on && x > l.max ? x : l.max;
        });
    });
    return expr_wave_reduce<T, OP>(l);
}

// one block per call: both columns' metadata and references and the lane's mask slices in flight together; only a block that keeps
// something requests packed rows, and only of the columns that have any
template <typename T>
__device__ __forceinline__ void aggregate_columns_block_wave(const AggregateColumnsArgs& a, uint64_t blk, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    const BlockLoads<T> la = issue_block_loads<T>(a, a.agg_refs, blk);
    const BlockLoads<T> lb = issue_block_loads<T>(a.b, a.b_refs, blk);
    uint32_t slice[M::GROUPS];
    block_mask_slices<T>(a.mask, blk, lane, slice);
    const BlockMeta ma = settle_block_loads<T>(a, blk, la);
    const BlockMeta mb = settle_block_loads<T>(a.b, blk, lb);
    if (const uint32_t err = ma.err | mb.err) {
        raise_device_error(a.err_flag, err, lane);
        store_block_aggregate(a, blk, aggregate_identity(), lane);
        return;
    }
    uint32_t any = 0;
    static_for<(int)M::GROUPS>([&](auto K) { any |= slice[decltype(K)::value]; });
    const bool empty = __builtin_amdgcn_ballot_w64(any != 0u) == 0ull;
    if (expr_route(empty ? 0u : 1u, ma.w, mb.w) <= EXPR_CONSTANT) {         // no packed load of either column (fl_expr_map.hpp)
        const unsigned count = empty ? 0u : aggregate_wave_count(aggregate_lane_of<T>(slice).count);
        store_block_aggregate(a, blk, expr_constant_block((int)a.expr, count, ma.r, mb.r), lane);
        return;
    }
    // EXPR_DECODE_A / _B / _BOTH in one path: wave-uniform descriptors over exactly each block's 128 * w bytes (a width-0 side: none,
    // nothing is requested of it)
    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.packed) + ma.off, 0, 128u * ma.w, 0x00020000);
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.b.packed) + mb.off, 0, 128u * mb.w, 0x00020000);
    const StagedRows<T> pk = request_image_and_staged<T>(ars, ma.w, brs, mb.w, lds, lane);
    wait_lds_dma();
    wave_lds_fence();
    // column a: the lane's 16 values into registers (W = 0: every field is 0, the value is the reference)
    Cell<T> va[G::GROUPS];
    const Cell<T> ca = Cell<T>::splat((T)ma.r);
    for_each_funnelled_cell<T>(ma.w, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) { va[decltype(K)::value] = cell.add(ca); });
    staged_to_image<T>(pk, mb.w, lds, lane);
    // column b through the same lane map, met with the kept values; the op is wave-uniform
    const T rb = (T)mb.r;
    BlockAggregate g;
    if (a.expr == EXPR_MUL) g = expr_lds_image<T, EXPR_MUL>(va, mb.w, lds, lane, rb, slice);
    else if (a.expr == EXPR_ADD) g = expr_lds_image<T, EXPR_ADD>(va, mb.w, lds, lane, rb, slice);
    else g = expr_lds_image<T, EXPR_SUB>(va, mb.w, lds, lane, rb, slice);
    store_block_aggregate(a, blk, g, lane);
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

template <typename T>
__global__ __launch_bounds__(WG) void k_unfor_aggregate_columns(AggregateColumnsArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        for (unsigned j = 0; j < count; ++j) aggregate_columns_block_wave<T>(a, first + j, lds, lane);
    });
}

typedef hipError_t (*aggregate_columns_launch_t)(const AggregateColumnsArgs&, int waves, hipStream_t);   // launch_block_consumer (fl_for_block.hpp)
template <typename T> aggregate_columns_launch_t aggregate_columns_launcher();

}  // namespace fl
