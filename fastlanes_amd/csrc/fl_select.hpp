// fl_select.hpp -- unfor_select: decode only the rows a selection mask keeps, from a FoR-packed column, uniform or mixed width.
// EXTENSION (SURVEY.md 8 f2 "unpack -> filter" / f4 "take"), defined as a composition of reference functions:
//     out = concat over b ascending of [ unfor_pack::<W_b>(block b, references[b * ref_stride])[i]  for i ascending if bit i of block b ]
// (ffor.rs:38-50; the mask in unpack_compare's layout: 32 words per block, bit i of block b = bit i % 32 of word b*32 + i/32, i in the
// unpacked index order).  Block b's run starts at out + out_offsets[b] (elements): the exclusive prefix sum of the blocks' popcounts
// (fl_scan.hpp: launch_mask_offsets), so no wavefront waits on another.  Delta columns are out of scope: a selected value needs its chain.
// The wave-per-block machinery of fl_widths.hpp and fl_for_compare.hpp:
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
#include "fl_widths.hpp"
#include "fl_for_compare.hpp"
#include "fl_select_map.hpp"

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
    constexpr int TB = G::TB;
    static_assert(M::GROUPS == (unsigned)G::GROUPS && M::N == (unsigned)Elem<T>::PER_CELL, "fl_select_map.hpp follows fl_widths.hpp's lane map");
    const unsigned c16 = (lane & 7u) * 16u;
    const typename G::word_t m = G::field_mask(w);
    unsigned bit = __umul24(G::row_base(lane >> 3), w);
    const unsigned step = G::KSTEP * w;
    const unsigned last = (w - 1u) * 128u;                                  // W = 0: wraps, the reads stay inside the image, m = 0
    const Cell<T> rc = Cell<T>::splat(ref);
    Cell<T> vals[G::GROUPS];
    static_for<G::GROUPS>([&](auto K) {
        const unsigned word = bit >> G::LOG_TB, sh = bit & (TB - 1u);
        const unsigned a0 = word * 128u;
        const unsigned a1 = a0 + 128u < last ? a0 + 128u : last;            // the last row never reads past the end (macros.rs:156)
        const Cell<T> cur = __builtin_bit_cast(Cell<T>, *reinterpret_cast<const u32x4*>(lds + a0 + c16));
        const Cell<T> nxt = __builtin_bit_cast(Cell<T>, *reinterpret_cast<const u32x4*>(lds + a1 + c16));
        vals[decltype(K)::value] = G::funnel(cur, nxt, sh, m).add(rc);     // ffor.rs:46-48
        bit += step;
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
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    constexpr int TB = G::TB;
    const unsigned z = opaque_zero();
    unsigned wv = a.uniform_width;
    uint64_t ov = 0;
    if (a.widths) wv = a.widths[blk + z];
    if (a.offsets) ov = a.offsets[blk + z];
    const T rv = static_cast<const T*>(a.sel_refs)[blk * a.ref_stride + z];
    const uint64_t dv = a.out_offsets[blk + z];
    BlockSelection<T> s;
    static_for<(int)M::GROUPS>([&](auto K) {
        constexpr unsigned k = decltype(K)::value;
        s.slice[k] = M::slice(a.mask[blk * SELECT_MASK_WORDS + M::mask_word(k, lane)], k, lane);
    });
    const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(wv);
    const uint64_t off = a.offsets ? wave_uniform_u64(ov) : blk * (uint64_t)(128u * w);
    const T r = (T)wave_uniform_u64((uint64_t)rv);
    const uint64_t dst = wave_uniform_u64(dv);
    if (const uint32_t e = block_precondition(a, w, off, TB)) {            // bitpacking.rs:126 unreachable!(), :111-113
        raise_device_error(a.err_flag, e, lane);
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
    if (w != 0u) {
        // wave-uniform descriptor over exactly this block's 128*w bytes: cells past it read as 0, no fault
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.packed) + off, 0, 128u * w, 0x00020000);
        Cell<T> no_ref;
        if (a.widths || w >= a.nt_from) packed_block_to_lds<T, RD_DMA_NT>(a, blk, rs, w, lds, lane, no_ref);   // RD_AUTO (fl_widths.hpp)
        else packed_block_to_lds<T, RD_VGPR>(a, blk, rs, w, lds, lane, no_ref);
        wave_lds_fence();
    }
    select_lds_image<T>(a, w, lds, lane, r, s, dst);
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

// the launch shapes select_blocks_wave_static serves (any other shape runs block by block through the wavefront's first image)
template <typename T> __host__ __device__ inline bool select_static_shape(unsigned bpw, unsigned prefetch)
{
    return sizeof(T) <= 2 && prefetch != 0u && (bpw == 2u || bpw == 4u);
}

// BPW consecutive blocks per wavefront (the narrow types' shipped shapes), as compare_blocks_wave_prefetched: lane j judges block
// first + j -- metadata, reference, preconditions -- and the wavefront reads the BPW masks (two blocks per load) into `stash`, BEFORE any
// packed load is issued; only the non-empty blocks' rows are then requested by LDS-DMA, one image per block, one wait, and the blocks
// are compacted back to back.  `stash`: BPW * 128 bytes of wave-private LDS behind the images.
template <typename T, unsigned BPW>
__device__ __forceinline__ void select_blocks_wave_static(const SelectArgs& a, uint64_t first, char* lds, uint32_t* stash, unsigned lane)
{
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    constexpr int TB = G::TB;
    static_assert(BPW >= 2 && BPW <= 16 && BPW % 2 == 0, "two blocks' masks per load");
    const bool owner = lane < BPW;
    const uint64_t mine = first + (owner ? lane : 0u);
    unsigned wv = a.uniform_width;
    if (a.widths) wv = a.widths[mine];
    uint64_t ov = mine * (uint64_t)(128u * wv);
    if (a.offsets) ov = a.offsets[mine];
    const T rv = static_cast<const T*>(a.sel_refs)[mine * a.ref_stride];
    const uint64_t dv = a.out_offsets[mine];
    uint32_t mw[BPW / 2];
    static_for<(int)(BPW / 2)>([&](auto I) {
        constexpr unsigned i = decltype(I)::value;
        mw[i] = a.mask[(first + 2u * i) * SELECT_MASK_WORDS + lane];        // words of blocks first + 2i (lanes 0..31) and first + 2i + 1
    });
    const uint32_t ev = block_precondition(a, wv, ov, TB);
    unsigned nonempty = 0;                                                  // wave-uniform: bit j = block first + j keeps something
    static_for<(int)(BPW / 2)>([&](auto I) {
        constexpr unsigned i = decltype(I)::value;
        stash[i * 64u + lane] = mw[i];
        const uint64_t nz = __builtin_amdgcn_ballot_w64(mw[i] != 0u);
        nonempty |= ((uint32_t)nz != 0u ? 1u : 0u) << (2u * i) | ((uint32_t)(nz >> 32) != 0u ? 2u : 0u) << (2u * i);
    });
    const uint64_t valid = __builtin_amdgcn_ballot_w64(owner && ev == 0u);
    const uint64_t fetch = valid & nonempty;
    static_for<(int)BPW>([&](auto J) {
        constexpr unsigned j = decltype(J)::value;
        if ((fetch >> j) & 1u) {
            const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)wv, (int)j);
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.packed) + readlane_u64(ov, j), 0, 128u * w, 0x00020000);
            char* img = lds + j * G::BLOCK_BYTES;
            static_for<G::GROUPS>([&](auto Gi) {
                constexpr int g = decltype(Gi)::value;
                if (8u * g < w) dma_1k_to_lds<RD_DMA_NT, g * 1024>(rs, img, lane);
            });
        }
    });
    wait_lds_dma();
    wave_lds_fence();
    for (unsigned j = 0; j < BPW; ++j) {                                    // wave-uniform loop
        if (const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)ev, (int)j)) {   // bitpacking.rs:126 unreachable!(), :111-113
            raise_device_error(a.err_flag, e, lane);
            continue;
        }
        if (!((nonempty >> j) & 1u)) continue;                              // empty mask: nothing was fetched, nothing is stored
        BlockSelection<T> s;
        static_for<(int)M::GROUPS>([&](auto K) {
            constexpr unsigned k = decltype(K)::value;
            s.slice[k] = M::slice(stash[j * SELECT_MASK_WORDS + M::mask_word(k, lane)], k, lane);
        });
        select_scan_block<T>(s, lane);
        const uint64_t dst = readlane_u64(dv, j);
        if (!select_run_inside(a, dst, s.count)) {
            raise_device_error(a.err_flag, DEVERR_BOUNDS, lane);
            continue;
        }
        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)wv, (int)j);
        select_lds_image<T>(a, w, lds + j * G::BLOCK_BYTES, lane, readlane_elem<T>(rv, j), s, dst);
    }
}

template <typename T>
__global__ __launch_bounds__(WG) void k_unfor_select(SelectArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        if constexpr (sizeof(T) <= 2) {                       // the shipped shapes of the narrow types; any other shape: block by block
            if (select_static_shape<T>(a.bpw, a.prefetch) && count == a.bpw) {
                extern __shared__ __attribute__((aligned(16))) char lds_all[];
                const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
                uint32_t* stash = reinterpret_cast<uint32_t*>(lds_all + (WG / 64) * WaveBlock<T>::BLOCK_BYTES * a.bpw) + wave * a.bpw * SELECT_MASK_WORDS;
                if (a.bpw == 4) select_blocks_wave_static<T, 4>(a, first, lds, stash, lane);
                else select_blocks_wave_static<T, 2>(a, first, lds, stash, lane);
                return;
            }
        }
        for (unsigned j = 0; j < count; ++j) select_block_wave<T>(a, first + j, lds, lane);
    });
}

// Launched with the shape of unfor_pack_widths (the C ABI passes fl_dispatch.hpp's mixed_* choices through with_policy); the tile map is
// plan_blocks', rotated for mixed-width columns as in launch_widths.  The masks' stash rides behind the workgroup's block images.
typedef hipError_t (*select_launch_t)(const SelectArgs&, int waves, hipStream_t);
template <typename T> hipError_t launch_unfor_select(const SelectArgs& a0, int waves, hipStream_t s)
{
    if (a0.n_blocks == 0) return hipSuccess;
    SelectArgs a = a0;
    const unsigned need = tidy_wave_blocks<T>(a.bpw, a.prefetch) + (select_static_shape<T>(a.bpw, a.prefetch) ? (WG / 64) * a.bpw * SELECT_MASK_WORDS * 4u : 0u);
    const unsigned grid = plan_blocks(a, a.n_blocks, a.bpw * (WG / 64), WIN_UNPACK, WaveBlock<T>::TB, a.widths != nullptr);
    const unsigned lds = occupancy_lds(waves, need);
    if (!grid || lds > 64 * 1024) return hipErrorInvalidValue;         // > 2^33 blocks; beyond the default dynamic-LDS limit
    FL_LAUNCH((k_unfor_select<T>), dim3(grid), dim3(WG), lds, s, a);
    return hipGetLastError();
}
template <typename T> select_launch_t select_launcher();

}  // namespace fl
