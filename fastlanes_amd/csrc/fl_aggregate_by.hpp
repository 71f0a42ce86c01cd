// fl_aggregate_by.hpp -- unfor_aggregate_by: COUNT / SUM / MIN / MAX of a FoR-packed VALUE column (u8 / u16 / u32 / u64) grouped by a
// FoR-packed u8 KEY column of the same block count, over the rows a selection mask keeps (no mask: every row).
// EXTENSION (SURVEY.md 8 f2 "unpack -> filter" followed by a grouped reduction), defined as a composition of reference functions:
//     val_b[i] = unfor_pack::<W_b >(value block b, references    [b * ref_stride    ])[i]          (ffor.rs:38-50)
//     key_b[i] = unfor_pack::<KW_b>(key   block b, key_references[b * key_ref_stride])[i]          (u8, wrapping add)
//     result[g] = combine over all (b, i) with mask bit (b, i) set and key_b[i] == g of {1, val, val, val}      (g = 0 .. 255)
// with the values zero-extended to 64 bits and combine / the identity {0, 0, UINT64_MAX, 0} those of fl_aggregate_map.hpp.  Integer
// add, min and max are associative and commutative: any order of the updates gives the same bits.
// One wavefront per workgroup, PERSISTENT (persistent_grid, fl_chain.hpp): a wavefront walks one contiguous run of blocks with a
// wave-private table of 256 BlockAggregate in LDS and flushes it once at its end.  Per block, through the steps of fl_for_block.hpp:
//   * both columns' width, offset and reference and the lane's mask slices arrive together (the NEXT block's are requested before this
//     block is worked on); both columns' preconditions are checked (block_precondition): a block that fails either raises its bits and
//     contributes nothing, neither column is read;
//   * the route comes from fl_aggregate_by_map.hpp (aggregate_by_route): an EMPTY mask reads nothing; key width 0 is unfor_aggregate's
//     block (aggregate_lds_image / aggregate_constant_block) folded into the slot of the key reference, no key byte read;
//   * otherwise both columns' rows are requested by LDS-DMA (one wait), the key block is decoded first and its 1024 keys stored to the
//     key area in index order, and lane l then funnels its cell of each 1-KiB group of the value block and reads the cell's N key bytes
//     with one ds_read (aggregate_by_key_byte);
//   * every kept element updates its key's slot with four LDS ATOMICS (two lanes of one instruction may hit the same key: a
//     read-modify-write through registers would lose updates).
// The flush: lane l takes groups l, l + 64, ..; a slot with count > 0 goes to result[g] with four relaxed agent-scope 64-bit vector
// atomics, behind k_aggregate_by_init (fl_scan.hpp) on the same stream, which writes the 256 identities.  No scratch memory.
// LDS is wave-local (in-order per wave): no s_barrier.  Every global store or atomic is a vector instruction.
#pragma once
#include "fl_aggregate.hpp"
#include "fl_aggregate_by_map.hpp"
#include "fl_chain.hpp"

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

// one update of the wavefront's table: LDS atomics, no value returned
__device__ __forceinline__ void group_table_update(BlockAggregate* table, unsigned key, uint64_t count, uint64_t sum, uint64_t lo, uint64_t hi)
{
    BlockAggregate* s = table + key;
    __hip_atomic_fetch_add(&s->count, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(&s->sum, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_min(&s->min, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_max(&s->max, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the wavefront's table after its last block -> result[256], which holds the identities or other wavefronts' flushes
__device__ __forceinline__ void group_table_flush(const BlockAggregate* table, BlockAggregate* result, unsigned lane)
{
    wave_lds_fence();
    for (unsigned g = lane; g < AGGREGATE_BY_GROUPS; g += 64u) {
        const BlockAggregate s = table[g];
        if (s.count != 0ull) {                                              // as k_aggregate_reduce: four 64-bit vector atomics
            BlockAggregate* out = result + g;
            __hip_atomic_fetch_add(&out->count, s.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&out->sum, s.sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(&out->min, s.min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&out->max, s.max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// a block's loads, issued and possibly still in flight
template <typename T> struct GroupBlockLoads {
    BlockLoads<T> v;
    BlockLoads<uint8_t> k;
    uint32_t slice[SelectMap<sizeof(T)>::GROUPS];
};
template <typename T> __device__ __forceinline__ GroupBlockLoads<T> aggregate_by_issue(const AggregateByArgs& a, uint64_t blk, unsigned lane)
{
    using M = SelectMap<sizeof(T)>;
    GroupBlockLoads<T> p;
    p.v = issue_block_loads<T>(a.val, a.val_refs, blk);
    p.k = issue_block_loads<uint8_t>(a.key, a.key_refs, blk);
    static_for<(int)M::GROUPS>([&](auto K) {
        constexpr unsigned k = decltype(K)::value;
        p.slice[k] = (1u << M::N) - 1u;                                     // no mask: every row
        if (a.mask) p.slice[k] = M::slice(a.mask[blk * SELECT_MASK_WORDS + M::mask_word(k, lane)], k, lane);
    });
    return p;
}

// the N key bytes of the lane's cell of group k, out of the key area: one aligned read
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
    // the key block first: its 1024 keys into the key area in index order, each lane's cell at 16 * lane
    Cell<uint8_t> keys = Cell<uint8_t>::zero();
    const Cell<uint8_t> krc = Cell<uint8_t>::splat((uint8_t)mk.r);
    for_each_funnelled_cell<uint8_t>(mk.w, key_lds, lane, [&](auto, unsigned, const Cell<uint8_t>& cell) { keys = cell.add(krc); });
    wave_lds_fence();                                                       // every lane holds its keys: the packed key rows are dead
    *reinterpret_cast<u32x4*>(key_lds + aggregate_by_key_store(lane)) = __builtin_bit_cast(u32x4, keys);
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
    group_table_flush(table, a.result, lane);
}

// Resident wavefronts per CU wanted; what fits the CU's LDS (17 / 13 / 11 / 10 KiB per wavefront for u64 / u32 / u16 / u8) caps it.
// `waves` (the A/B tools' occupancy knob: waves per SIMD) overrides it.
constexpr int AGGREGATE_BY_WAVES_PER_CU = 16;

// The grid is what is resident at once, at most one wavefront per block; a wavefront's run is the column divided evenly, and at least
// `bpw` blocks (the A/B tools' and the tests' blocks-per-wavefront override; 0 = none).  The caller has launched k_aggregate_by_init.
// KERNEL takes Args, which has a `run` field; LDS is its request per wavefront.
template <auto KERNEL, unsigned LDS, typename Args>
hipError_t launch_group_runs(Args a, uint64_t n, unsigned bpw, int waves, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    static_assert(LDS <= 64 * 1024, "the default dynamic-LDS limit");
    unsigned grid = n < (1ull << 30) ? (unsigned)n : 1u << 30;
    if (hipError_t e = persistent_grid<KERNEL>(LDS, waves > 0 ? 4 * waves : AGGREGATE_BY_WAVES_PER_CU, grid); e != hipSuccess) return e;
    a.run = (n + grid - 1) / grid;
    if (a.run < bpw) a.run = bpw;
    FL_LAUNCH(KERNEL, dim3(grid), dim3(64), LDS, s, a);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_aggregate_by(const AggregateByArgs& a, int waves, hipStream_t s)
{
    return launch_group_runs<k_unfor_aggregate_by<T>, aggregate_by_lds<T>()>(a, a.val.n_blocks, a.val.bpw, waves, s);
}

typedef hipError_t (*aggregate_by_launch_t)(const AggregateByArgs&, int waves, hipStream_t);
template <typename T> aggregate_by_launch_t aggregate_by_launcher();

}  // namespace fl
