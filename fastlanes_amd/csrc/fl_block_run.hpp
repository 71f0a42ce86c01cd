// fl_block_run.hpp -- the pieces the six RUN-WALKING consumers of a FoR-packed column share: unfor_aggregate_by (fl_aggregate_by.hpp),
// unfor_aggregate_by_columns, unfor_aggregate_by_window, unfor_aggregate_by_lookup, unfor_set_build (fl_set_build.hpp) and unfor_lookup
// (fl_lookup.hpp); the wave-per-block aggregates and unfor_compare_columns use the mask slices and the two-column fetch.  Built on
// fl_for_block.hpp.
// The skeleton of a run-walking kernel: one wavefront per workgroup, PERSISTENT (launch_group_runs; persistent_grid, fl_chain.hpp).
// Workgroup g owns the contiguous run of blocks [g * run, (g + 1) * run); one that owns none returns before it touches LDS and flushes
// nothing.  The run is walked ONE BLOCK AHEAD: the kernel's `issue` (issue_block_loads of every column, block_mask_slices) requests
// the NEXT block's metadata, references and mask slices before its `block` works on this one, and the run's last block asks for itself
// again, which keeps the loop straight-line.  What a wavefront gathers over its run is flushed ONCE at its end:
//   * a wave-private table of BlockAggregate in LDS, its slots initialised to {0, 0, UINT64_MAX, 0}, updated with LDS atomics
//     (group_table_update: two lanes of one instruction may hit the same slot, a read-modify-write through registers would lose
//     updates) and flushed slot by slot, lane l taking slots l, l + 64, .. (group_table_flush; the window kernel's flush goes into
//     its own arrays): only a slot with count > 0 is written, so a wavefront adds nothing to groups it never met;
//   * two per-lane counters, folded over the wavefront (wave_sum_u64) and added with at most two 64-bit vector atomics.
// Each kernel writes its own run loop, table initialisation and counter tail: as shared functions (a walker taking the kernel's issue
// and block as callables, an init function, a counter-pair function, a flush taking a sink) each of them changed the instructions the
// compiler emits for the kernels -- reordered pairs, inverted branches, 5 more SGPRs in one -- and what is shared here is what left
// every kernel identical, at most up to register names, to what it was with its own copy.
// Two columns of one element type meet through ONE image (request_image_and_staged / staged_to_image): a lane's cell of group k holds
// the same row indices in either.  (unfor_aggregate_by_columns keeps its own copy of that fetch, for the same reason.)
// Everything here but the launcher is inlined into its kernel.  LDS is wave-local (in-order per wave): no s_barrier, and no LDS of
// this header's own.  Every global store or atomic is a vector instruction.
#pragma once
#include "fl_for_block.hpp"
#include "fl_chain.hpp"
#include "fl_aggregate_map.hpp"

namespace fl {

// The lane's slices of block `blk`'s mask, one per 1-KiB group (mask == nullptr: every row is kept, no mask is read).  The wave-uniform
// "no lane keeps a row" test that follows them stays in each kernel: behind a function boundary the compiler keeps the slices in a
// vector register and every consumer came out with more VGPRs and other code.
template <typename T>
__device__ __forceinline__ void block_mask_slices(const uint32_t* const& mask, const uint64_t& blk, unsigned lane, uint32_t (&slice)[SelectMap<sizeof(T)>::GROUPS])
{
    using M = SelectMap<sizeof(T)>;
    static_for<(int)M::GROUPS>([&](auto K) {
        constexpr unsigned k = decltype(K)::value;
        slice[k] = (1u << M::N) - 1u;                                       // no mask: every row
        if (mask) slice[k] = M::slice(mask[blk * SELECT_MASK_WORDS + M::mask_word(k, lane)], k, lane);
    });
}

// one update of the wavefront's table: LDS atomics, no value returned
__device__ __forceinline__ void group_table_update(BlockAggregate* table, unsigned key, uint64_t count, uint64_t sum, uint64_t lo, uint64_t hi)
{
    BlockAggregate* s = table + key;
    __hip_atomic_fetch_add(&s->count, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(&s->sum, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_min(&s->min, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_max(&s->max, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the wavefront's table after its last block -> result[n_slots], which holds the identities (k_aggregate_by_init, fl_scan.hpp, on the
// same stream) or other wavefronts' flushes: only what this wavefront has updated, with four relaxed agent-scope 64-bit vector atomics,
// as k_aggregate_reduce
__device__ __forceinline__ void group_table_flush(const BlockAggregate* table, unsigned n_slots, BlockAggregate* result, unsigned lane)
{
    wave_lds_fence();
    for (unsigned g = lane; g < n_slots; g += 64u) {
        const BlockAggregate s = table[g];
        if (s.count != 0ull) {
            BlockAggregate* out = result + g;
            __hip_atomic_fetch_add(&out->count, s.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&out->sum, s.sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(&out->min, s.min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&out->max, s.max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// a per-lane counter folded over the wavefront, in every lane
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Two blocks of one element type through ONE image: column x's x_w rows are requested by LDS-DMA into the image, column y's y_w rows
// into the staging registers pk[] (non-temporal, as the DMA); the descriptors cover exactly each block's 128 * w bytes, a width-0 column
// requests nothing.  The caller adds any request of its own, then waits once: wait_lds_dma(); wave_lds_fence();
// pk[] travels BY VALUE: the rows of a group that requested nothing stay undefined and are never read, and handed out by reference the
// compiler zeroes them instead (four v_mov per group and a branch).
template <typename T> struct StagedRows {
    u32x4 pk[WaveBlock<T>::GROUPS];
};
template <typename T>
__device__ __forceinline__ StagedRows<T> request_image_and_staged(const __amdgpu_buffer_rsrc_t& x_rsrc, unsigned x_w, const __amdgpu_buffer_rsrc_t& y_rsrc,
                                                                  unsigned y_w, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    StagedRows<T> st;
    static_for<G::GROUPS>([&](auto Gi) {
        constexpr int g = decltype(Gi)::value;
        if (8u * g < x_w) dma_1k_to_lds<RD_DMA_NT, g * 1024>(x_rsrc, lds, lane);
    });
    static_for<G::GROUPS>([&](auto Gi) {
        constexpr int g = decltype(Gi)::value;
        if (8u * g < y_w) st.pk[g] = __builtin_amdgcn_raw_buffer_load_b128(y_rsrc, lane * 16u + g * 1024u, 0, 2);
    });
    return st;
}
// once every lane holds what it needs of column x, the image is dead: column y's staged rows overwrite it, ready to be funnelled
template <typename T>
__device__ __forceinline__ void staged_to_image(const StagedRows<T>& st, unsigned y_w, char* lds, unsigned lane)
{
    wave_lds_fence();
    static_for<WaveBlock<T>::GROUPS>([&](auto Gi) {
        constexpr int g = decltype(Gi)::value;
        if (8u * g < y_w) *reinterpret_cast<u32x4*>(lds + lane * 16u + g * 1024u) = st.pk[g];
    });
    wave_lds_fence();
}

// Resident wavefronts per CU wanted; what fits the CU's LDS (for unfor_aggregate_by 17 / 13 / 11 / 10 KiB per wavefront for u64 / u32 /
// u16 / u8) caps it.  `waves` (the A/B tools' occupancy knob: waves per SIMD) overrides it.
constexpr int GROUP_RUN_WAVES_PER_CU = 16;

// The grid is what is resident at once, at most one wavefront per block; a wavefront's run is the column divided evenly, and at least
// `bpw` blocks (the A/B tools' and the tests' blocks-per-wavefront override; 0 = none).  KERNEL takes Args, which has a `run` field; LDS
// is its request per wavefront.
template <auto KERNEL, unsigned LDS, typename Args>
hipError_t launch_group_runs(Args a, uint64_t n, unsigned bpw, int waves, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    static_assert(LDS <= 64 * 1024, "the default dynamic-LDS limit");
    unsigned grid = n < (1ull << 30) ? (unsigned)n : 1u << 30;
    if (hipError_t e = persistent_grid<KERNEL>(LDS, waves > 0 ? 4 * waves : GROUP_RUN_WAVES_PER_CU, grid); e != hipSuccess) return e;
    a.run = (n + grid - 1) / grid;
    if (a.run < bpw) a.run = bpw;
    FL_LAUNCH(KERNEL, dim3(grid), dim3(64), LDS, s, a);
    return hipGetLastError();
}

}  // namespace fl
