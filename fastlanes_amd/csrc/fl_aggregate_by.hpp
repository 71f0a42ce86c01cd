// fl_aggregate_by.hpp -- unfor_aggregate_by: COUNT / SUM / MIN / MAX of a FoR-packed VALUE column (u8 / u16 / u32 / u64) grouped by a
// FoR-packed u8 KEY column of the same block count, over the rows a selection mask keeps (no mask: every row).
// EXTENSION (SURVEY.md 8 f2 "unpack -> filter" followed by a grouped reduction), defined as a composition of reference functions:
//     val_b[i] = unfor_pack::<W_b >(value block b, references    [b * ref_stride    ])[i]          (ffor.rs:38-50)
//     key_b[i] = unfor_pack::<KW_b>(key   block b, key_references[b * key_ref_stride])[i]          (u8, wrapping add)
//     result[g] = combine over all (b, i) with mask bit (b, i) set and key_b[i] == g of {1, val, val, val}      (g = 0 .. 255)
// with the values zero-extended to 64 bits and combine / the identity {0, 0, UINT64_MAX, 0} those of fl_aggregate_map.hpp.  Integer
// add, min and max are associative and commutative: any order of the updates gives the same bits.
// A run-walking kernel (fl_block_run.hpp: the run, the one-block look-ahead, the wave-private table of 256 BlockAggregate and its flush
// into result[256], behind k_aggregate_by_init, fl_scan.hpp, on the same stream).  Per block, through the steps of fl_for_block.hpp:
//   * both columns' preconditions are checked (block_precondition): a block that fails either raises its bits and contributes nothing,
//     neither column is read;
//   * the route comes from fl_aggregate_by_map.hpp (aggregate_by_route): an EMPTY mask reads nothing; key width 0 is unfor_aggregate's
//     block (aggregate_lds_image / aggregate_constant_block) folded into the slot of the key reference, no key byte read;
//   * otherwise both columns' rows are requested by LDS-DMA (one wait), the key block is decoded first and its 1024 keys stored to the
//     key area in index order, and lane l then funnels its cell of each 1-KiB group of the value block and reads the cell's N key bytes
//     with one ds_read (aggregate_by_key_byte);
//   * every kept element updates its key's slot (group_table_update).
// No scratch memory.
// LDS is wave-local (in-order per wave): no s_barrier.  Every global store or atomic is a vector instruction.
#pragma once
#include "fl_aggregate.hpp"
#include "fl_aggregate_by_map.hpp"

namespace fl {

// WidthsArgs::refs and ::unpacked stay nullptr in both columns: the references are loaded with the blocks' metadata
struct AggregateByArgs {
    WidthsArgs val, key;           // the same n_blocks, the same err_flag
    const void* val_refs;          // references[b * val.ref_stride]
    const void* key_refs;          // key_references[b * key.ref_stride]
    const uint32_t* mask;          // [n_blocks][32]; nullptr = every row is kept (no mask is read)
    BlockAggregate* result;        // [256]
    uint64_t run;                  // blocks of a wavefront's run; filled by the launcher
};

template <typename T> constexpr unsigned aggregate_by_lds() { return aggregate_by_wave_lds(WaveBlock<T>::BLOCK_BYTES); }

// a block's loads, issued and possibly still in flight
template <typename T> struct GroupBlockLoads {
    BlockLoads<T> v;
    BlockLoads<uint8_t> k;
    uint32_t slice[SelectMap<sizeof(T)>::GROUPS];
};
template <typename T> __device__ __forceinline__ GroupBlockLoads<T> aggregate_by_issue(const AggregateByArgs& a, uint64_t blk, unsigned lane)
{
    GroupBlockLoads<T> p;
    p.v = issue_block_loads<T>(a.val, a.val_refs, blk);
    p.k = issue_block_loads<uint8_t>(a.key, a.key_refs, blk);
    block_mask_slices<T>(a.mask, blk, lane, p.slice);
    return p;
}

// The key area (fl_aggregate_by_map.hpp), shared with unfor_aggregate_by_columns.  The packed rows of a u8 key block of width
// 1 <= kw <= 8 in it -> its 1024 keys (reference added) in index order, the lane's cell at 16 * lane.  The caller fences before the keys
// are read.
__device__ __forceinline__ void decode_keys_to_area(unsigned kw, uint8_t kref, char* key_lds, unsigned lane)
{
    Cell<uint8_t> keys = Cell<uint8_t>::zero();
    const Cell<uint8_t> krc = Cell<uint8_t>::splat(kref);
    for_each_funnelled_cell<uint8_t>(kw, key_lds, lane, [&](auto, unsigned, const Cell<uint8_t>& cell) { keys = cell.add(krc); });
    wave_lds_fence();                                                       // every lane holds its keys: the packed key rows are dead
    *reinterpret_cast<u32x4*>(key_lds + aggregate_by_key_store(lane)) = __builtin_bit_cast(u32x4, keys);
}
// the N key bytes of the lane's cell of group k of a block of T, out of the key area: one aligned read
template <typename T> __device__ __forceinline__ void cell_keys(const char* key_lds, unsigned k, unsigned lane, uint32_t (&kw)[4])
{
    constexpr unsigned N = SelectMap<sizeof(T)>::N;
    const char* at = key_lds + aggregate_by_key_byte<sizeof(T)>(k, lane, 0u);
    if constexpr (N == 16) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(at);
        kw[0] = q.x; kw[1] = q.y; kw[2] = q.z; kw[3] = q.w;
    } else if constexpr (N == 8) {
        const uint64_t q = *reinterpret_cast<const uint64_t*>(at);
        kw[0] = (uint32_t)q; kw[1] = (uint32_t)(q >> 32);
    } else if constexpr (N == 4) {
        kw[0] = *reinterpret_cast<const uint32_t*>(at);
    } else {
        kw[0] = *reinterpret_cast<const uint16_t*>(at);
    }
}

// one block whose loads were issued by aggregate_by_issue.  lds: [value image | key area | table]
template <typename T>
__device__ __forceinline__ void aggregate_by_block(const AggregateByArgs& a, uint64_t blk, const GroupBlockLoads<T>& p, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    char* key_lds = lds + G::BLOCK_BYTES;
    BlockAggregate* table = reinterpret_cast<BlockAggregate*>(key_lds + AGGREGATE_BY_KEY_BYTES);
    const BlockMeta mv = settle_block_loads<T>(a.val, blk, p.v);
    const BlockMeta mk = settle_block_loads<uint8_t>(a.key, blk, p.k);
    uint32_t any = 0;
    static_for<(int)M::GROUPS>([&](auto K) { any |= p.slice[decltype(K)::value]; });
    const bool empty = __builtin_amdgcn_ballot_w64(any != 0u) == 0ull;
    const uint32_t err = mv.err | mk.err;
    if (err) raise_device_error(a.val.err_flag, err, lane);
    const AggregateByRoute route = aggregate_by_route(empty, err == 0u, mk.w);
    if (route == AGGBY_SKIP) return;
    const T r = (T)mv.r;
    if (route == AGGBY_ONE_KEY) {                                           // unfor_aggregate's block, folded into one slot
        BlockAggregate g;
        if (!aggregate_by_reads_values(route, mv.w)) {
            g = aggregate_constant_block(aggregate_wave_count(aggregate_lane_of<T>(p.slice).count), (uint64_t)r);
        } else {
            fill_block_image<T>(a.val, blk, mv.off, mv.w, lds, lane);
            g = aggregate_lds_image<T>(mv.w, lds, lane, r, p.slice);
            wave_lds_fence();                                               // the image is reused by the wavefront's next block
        }
        if (lane == 0u) group_table_update(table, (unsigned)mk.r & 0xffu, g.count, g.sum, g.min, g.max);
        return;
    }
    // both columns' rows by LDS-DMA, one wait; wave-uniform descriptors over exactly each block's bytes (a width-0 value block: none)
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.val.packed) + mv.off, 0, 128u * mv.w, 0x00020000);
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.key.packed) + mk.off, 0, 128u * mk.w, 0x00020000);
    static_for<G::GROUPS>([&](auto Gi) {
        constexpr int g = decltype(Gi)::value;
        if (8u * g < mv.w) dma_1k_to_lds<RD_DMA_NT, g * 1024>(vrs, lds, lane);
    });
    dma_1k_to_lds<RD_DMA_NT, 0>(krs, key_lds, lane);                        // 1 <= key width <= 8: one KiB, bytes past the block arrive as 0
    wait_lds_dma();
    wave_lds_fence();
    decode_keys_to_area(mk.w, (uint8_t)mk.r, key_lds, lane);                // the key block first
    wave_lds_fence();
    const Cell<T> rc = Cell<T>::splat(r);
    for_each_funnelled_cell<T>(mv.w, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) {
        constexpr unsigned k = decltype(K)::value;
        const Cell<T> v = cell.add(rc);                                     // ffor.rs:46-48
        const uint32_t sl = p.slice[k];
        uint32_t kw[4];
        cell_keys<T>(key_lds, k, lane, kw);
        static_for<(int)M::N>([&](auto E) {
            constexpr unsigned e = decltype(E)::value;
            if ((sl >> e) & 1u) {
                const uint64_t x = cell_get<T>(v, (int)e);
                group_table_update(table, (kw[e / 4u] >> (8u * (e % 4u))) & 0xffu, 1ull, x, x, x);
            }
        });
    });
    wave_lds_fence();                                                       // image and key area are reused by the wavefront's next block
}

// Workgroup (= wavefront) g owns blocks [g * run, (g + 1) * run) of the column; one that owns none returns at once.
template <typename T>
__global__ __launch_bounds__(64) void k_unfor_aggregate_by(AggregateByArgs a)
{
    using G = WaveBlock<T>;
    extern __shared__ __attribute__((aligned(16))) char lds_all[];
    const unsigned lane = threadIdx.x;
    const uint64_t n = a.val.n_blocks;
    const uint64_t first = (uint64_t)blockIdx.x * a.run;
    if (first >= n) return;
    const uint64_t end = n - first < a.run ? n : first + a.run;
    BlockAggregate* table = reinterpret_cast<BlockAggregate*>(lds_all + G::BLOCK_BYTES + AGGREGATE_BY_KEY_BYTES);
    for (unsigned g = lane; g < AGGREGATE_BY_GROUPS; g += 64u) {
        u32x4* s = reinterpret_cast<u32x4*>(table + g);
        s[0] = u32x4{0u, 0u, 0u, 0u};                                       // count, sum
        s[1] = u32x4{~0u, ~0u, 0u, 0u};                                     // min, max
    }
    wave_lds_fence();
    GroupBlockLoads<T> cur = aggregate_by_issue<T>(a, first, lane);
    for (uint64_t blk = first; blk < end; ++blk) {                          // wave-uniform loop
        const uint64_t ahead = blk + 1 < end ? blk + 1 : blk;               // the last block asks for itself again: straight-line code
        const GroupBlockLoads<T> nxt = aggregate_by_issue<T>(a, ahead, lane);
        aggregate_by_block<T>(a, blk, cur, lds_all, lane);
        cur = nxt;
    }
    group_table_flush(table, AGGREGATE_BY_GROUPS, a.result, lane);
}

template <typename T>
hipError_t launch_aggregate_by(const AggregateByArgs& a, int waves, hipStream_t s)
{
    return launch_group_runs<k_unfor_aggregate_by<T>, aggregate_by_lds<T>()>(a, a.val.n_blocks, a.val.bpw, waves, s);
}

typedef hipError_t (*aggregate_by_launch_t)(const AggregateByArgs&, int waves, hipStream_t);
template <typename T> aggregate_by_launch_t aggregate_by_launcher();

}  // namespace fl
