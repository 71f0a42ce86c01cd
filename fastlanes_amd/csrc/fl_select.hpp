// fl_select.hpp -- unfor_select: decode only the rows a selection mask keeps, from a FoR-packed column, uniform or mixed width.
// EXTENSION (SURVEY.md 8 f2 "unpack -> filter" / f4 "take"), defined as a composition of reference functions:
//     out = concat over b ascending of [ unfor_pack::<W_b>(block b, references[b * ref_stride])[i]  for i ascending if bit i of block b ]
// (ffor.rs:38-50; the mask in unpack_compare's layout: 32 words per block, bit i of block b = bit i % 32 of word b*32 + i/32, i in the
// unpacked index order).  Block b's run starts at out + out_offsets[b] (elements): the exclusive prefix sum of the blocks' popcounts
// (fl_scan.hpp: launch_mask_offsets), so no wavefront waits on another.  A Delta-packed column has undelta_select (fl_delta_select.hpp).
// The wave-per-block machinery of fl_widths.hpp, through the steps fl_for_block.hpp shares among the four consumers of a packed column:
//   * a block's width, offset, reference, out_offsets[b] AND its 128-byte mask arrive together (independent vector loads, one wait);
//     its preconditions are checked (block_precondition: a failing block is skipped, its output slots untouched), and a block whose
//     run does not lie inside [0, out_len) is skipped with FL_DEVERR_BOUNDS -- a wrong offsets array never writes outside `out`;
//   * a block whose mask is EMPTY issues no packed load and no store;
//   * any other block fills its LDS image as unpack_widths does; lane l funnels its cell of each 1-KiB group, adds the reference, and
//     writes its kept elements into the (by then dead) image at the positions fl_select_map.hpp gives -- one wave scan of the lanes'
//     packed per-group counts -- so that the run stands contiguous in LDS, in index order;
//   * the run leaves coalesced, one element per lane per store, through a descriptor of exactly count * sizeof(T) bytes: the destination
//     is only element-aligned and the neighbouring bytes belong to other wavefronts.
// LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_for_compare.hpp"

namespace fl {

// WidthsArgs::refs and ::unpacked stay nullptr: the reference is loaded with the block's metadata, the output is the compacted column
struct SelectArgs : WidthsArgs {
    const uint32_t* mask;          // [n_blocks][32]
    const uint64_t* out_offsets;   // [n_blocks], elements
    char* out;                     // out_len elements
    uint64_t out_len;
    const void* sel_refs;          // references[b * ref_stride]
};

template <typename T> struct SelectScan {
    using M = SelectMap<sizeof(T)>;
    using word_t = std::conditional_t<M::SCAN_BITS == 32, uint32_t, uint64_t>;
};

// what a wavefront knows of a block's mask: each lane's slices, its exclusive scan value, the groups' totals
template <typename T> struct BlockSelection {
    uint32_t slice[SelectMap<sizeof(T)>::GROUPS];
    uint64_t excl, totals;
    unsigned count;                // wave-uniform
};

// inclusive scan over the 64 lanes of the packed per-group counts (no field carries into the next: fl_select_map.hpp)
template <typename W> __device__ __forceinline__ W select_wave_incl_scan(W v, unsigned lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const W o = __shfl_up(v, d, 64);
        if (lane >= (unsigned)d) v += o;
    }
    return v;
}

// slices (already cut out of the mask words) -> the block's selection
template <typename T> __device__ __forceinline__ void select_scan_block(BlockSelection<T>& s, unsigned lane)
{
    using M = SelectMap<sizeof(T)>;
    using word_t = typename SelectScan<T>::word_t;
    word_t mine = 0;
    static_for<(int)M::GROUPS>([&](auto K) {
        constexpr unsigned k = decltype(K)::value;
        mine |= (word_t)M::pack_count((unsigned)__builtin_popcount(s.slice[k]), k);
    });
    const word_t incl = select_wave_incl_scan<word_t>(mine, lane);
    s.excl = incl - mine;
    if constexpr (sizeof(word_t) == 8) s.totals = readlane_u64(incl, 63u);
    else s.totals = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    s.count = M::group_base(s.totals, M::GROUPS);
}

// true if the block's run [dst, dst + count) lies inside the output
__device__ __forceinline__ bool select_run_inside(const SelectArgs& a, uint64_t dst, unsigned count)
{
    return dst <= a.out_len && count <= a.out_len - dst;
}

typedef uint32_t select_u32x2 __attribute__((ext_vector_type(2)));
template <typename T> __device__ __forceinline__ void select_store_elem(T v, __amdgpu_buffer_rsrc_t rs, unsigned byte_off)
{
    if constexpr (sizeof(T) == 1) __builtin_amdgcn_raw_buffer_store_b8(v, rs, byte_off, 0, STORE_AUX);
    else if constexpr (sizeof(T) == 2) __builtin_amdgcn_raw_buffer_store_b16(v, rs, byte_off, 0, STORE_AUX);
    else if constexpr (sizeof(T) == 4) __builtin_amdgcn_raw_buffer_store_b32(v, rs, byte_off, 0, STORE_AUX);
    else __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(select_u32x2, v), rs, byte_off, 0, STORE_AUX);
}

// The LDS image of a non-empty block (w rows; w = 0: nothing was fetched, the field mask is 0 and every value is the reference) -> its
// run at out + dst.  Requires select_run_inside(a, dst, s.count).
template <typename T>
__device__ __forceinline__ void select_lds_image(const SelectArgs& a, unsigned w, char* lds, unsigned lane, T ref, const BlockSelection<T>& s, uint64_t dst)
{
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    static_assert(M::GROUPS == (unsigned)G::GROUPS && M::N == (unsigned)Elem<T>::PER_CELL, "fl_select_map.hpp follows fl_widths.hpp's lane map");
    const Cell<T> rc = Cell<T>::splat(ref);
    Cell<T> vals[G::GROUPS];
    for_each_funnelled_cell<T>(w, lds, lane, [&](auto K, unsigned bit, const Cell<T>& cell) {
        vals[decltype(K)::value] = cell.add(rc);                            // ffor.rs:46-48
    });
    wave_lds_fence();                                                       // every lane holds its cells: the image is dead
    T* run = reinterpret_cast<T*>(lds);
    static_for<G::GROUPS>([&](auto K) {
        constexpr unsigned k = decltype(K)::value;
        const uint32_t sl = s.slice[k];
        unsigned at = M::landing(s.totals, s.excl, k, sl, 0u);
        static_for<(int)M::N>([&](auto E) {
            constexpr unsigned e = decltype(E)::value;
            if ((sl >> e) & 1u) run[at] = (T)cell_get<T>(vals[k], (int)e);
            at += (sl >> e) & 1u;
        });
    });
    wave_lds_fence();
    // exactly this block's count * sizeof(T) bytes: lanes past the run's end are dropped by the descriptor
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.out + dst * sizeof(T), 0, s.count * (unsigned)sizeof(T), 0x00020000);
    for (unsigned i0 = 0; i0 < s.count; i0 += 64u) {                        // wave-uniform trip count; i0 + lane < 1024: inside the image
        const unsigned i = i0 + lane;
        select_store_elem<T>(run[i], rs, i * (unsigned)sizeof(T));
    }
}

// one block per call: metadata, reference, out_offsets[b] and the lane's mask slices in flight together
template <typename T>
__device__ __forceinline__ void select_block_wave(const SelectArgs& a, uint64_t blk, char* lds, unsigned lane)
{
    using M = SelectMap<sizeof(T)>;
    const BlockLoads<T> loads = issue_block_loads<T>(a, a.sel_refs, blk);
    const uint64_t dv = a.out_offsets[blk + loads.z];
    BlockSelection<T> s;
    static_for<(int)M::GROUPS>([&](auto K) {
        constexpr unsigned k = decltype(K)::value;
        s.slice[k] = M::slice(a.mask[blk * SELECT_MASK_WORDS + M::mask_word(k, lane)], k, lane);
    });
    const BlockMeta m = settle_block_loads<T>(a, blk, loads);
    const uint64_t dst = wave_uniform_u64(dv);
    if (m.err) {
        raise_device_error(a.err_flag, m.err, lane);
        return;
    }
    uint32_t any = 0;
    static_for<(int)M::GROUPS>([&](auto K) { any |= s.slice[decltype(K)::value]; });
    if (__builtin_amdgcn_ballot_w64(any != 0u) == 0ull) return;             // empty mask: no packed load, no store
    select_scan_block<T>(s, lane);
    if (!select_run_inside(a, dst, s.count)) {
        raise_device_error(a.err_flag, DEVERR_BOUNDS, lane);
        return;
    }
    if (m.w != 0u) fill_block_image<T>(a, blk, m.off, m.w, lds, lane);
    select_lds_image<T>(a, m.w, lds, lane, (T)m.r, s, dst);
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

// BPW consecutive blocks per wavefront (the narrow types' shipped shapes: static_shape), as compare_blocks_wave_prefetched: lane j judges
// block first + j -- metadata, reference, preconditions -- and the wavefront reads the BPW masks into its stash, BEFORE any packed load
// is issued; only the non-empty blocks' rows are then requested by LDS-DMA, one image per block, one wait, and the blocks are compacted
// back to back.
template <typename T, unsigned BPW>
__device__ __forceinline__ void select_blocks_wave_static(const SelectArgs& a, uint64_t first, char* lds, uint32_t* stash, unsigned lane)
{
    using G = WaveBlock<T>;
    const LaneBlocks<T> l = lane_block_loads<T>(a, a.sel_refs, first, BPW, lane);
    const uint64_t dv = a.out_offsets[l.mine];
    const unsigned nonempty = stash_block_masks<BPW>(a.mask, first, stash, lane);
    request_block_images<T, BPW>(a, l, __builtin_amdgcn_ballot_w64(l.owner && l.ev == 0u) & nonempty, lds, lane);
    for (unsigned j = 0; j < BPW; ++j) {                                    // wave-uniform loop
        if (const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)l.ev, (int)j)) {
            raise_device_error(a.err_flag, e, lane);
            continue;
        }
        if (!((nonempty >> j) & 1u)) continue;                              // empty mask: nothing was fetched, nothing is stored
        BlockSelection<T> s;
        stashed_slices<T>(stash, j, lane, s.slice);
        select_scan_block<T>(s, lane);
        const uint64_t dst = readlane_u64(dv, j);
        if (!select_run_inside(a, dst, s.count)) {
            raise_device_error(a.err_flag, DEVERR_BOUNDS, lane);
            continue;
        }
        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)l.wv, (int)j);
        select_lds_image<T>(a, w, lds + j * G::BLOCK_BYTES, lane, readlane_elem<T>(l.rv, j), s, dst);
    }
}

template <typename T>
__global__ __launch_bounds__(WG) void k_unfor_select(SelectArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        if constexpr (sizeof(T) <= 2) {                       // the shipped shapes of the narrow types; any other shape: block by block
            if (static_shape<T>(a.bpw, a.prefetch) && count == a.bpw) {
                uint32_t* stash = wave_mask_stash<T>(a.bpw);
                if (a.bpw == 4) select_blocks_wave_static<T, 4>(a, first, lds, stash, lane);
                else select_blocks_wave_static<T, 2>(a, first, lds, stash, lane);
                return;
            }
        }
        for (unsigned j = 0; j < count; ++j) select_block_wave<T>(a, first + j, lds, lane);
    });
}

typedef hipError_t (*select_launch_t)(const SelectArgs&, int waves, hipStream_t);   // launch_block_consumer (fl_for_block.hpp), with the stash
template <typename T> select_launch_t select_launcher();

}  // namespace fl
