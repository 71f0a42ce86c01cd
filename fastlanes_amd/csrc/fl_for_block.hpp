// fl_for_block.hpp -- the steps the four consumers of a FoR-packed column share: unfor_compare (fl_for_compare.hpp), unfor_compare_range
// (fl_for_compare_range.hpp), unfor_select (fl_select.hpp) and unfor_aggregate (fl_aggregate.hpp).  Each of them is the wave-per-block
// machinery of fl_widths.hpp with something other than a store of the decoded block at its end, so each goes through the same steps:
//   * ONE block per call: issue_block_loads (width, offset, reference as independent vector loads), the kernel's own loads behind them,
//     settle_block_loads (one wait, wave-uniform values, the preconditions), fill_block_image (the packed rows into the LDS image);
//   * SEVERAL blocks per wavefront: lane_block_loads (lane j holds block first + j's metadata and preconditions), request_block_images
//     (LDS-DMA for the blocks of a wave-uniform mask, one wait); select and aggregate keep the blocks' mask words in a wave-private
//     stash behind the images meanwhile (static_shape, wave_mask_stash, stash_block_masks, stashed_slices);
//   * for_each_funnelled_cell walks a block's LDS image, the lane's cell of every 1-KiB group; verdicts_to_image gathers one verdict bit
//     per element into the first 128 bytes of the (by then dead) image;
//   * launch_block_consumer launches any of the four kernels with the shape of unfor_pack_widths.
// unpack_widths itself (fl_widths.hpp) keeps its own copy of these steps: its kernels carry the headline figures and stay as they are.
// LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_widths.hpp"
#include "fl_consume.hpp"
#include "fl_select_map.hpp"

namespace fl {

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, unsigned j)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j);
}

// The LDS image of a block of w rows: f(K, bit, cell) for every 1-KiB group K (a static_for index) with `bit` = the bit position of the
// lane's row in every FL lane's stream and `cell` = its 16/sizeof(T) fields, no reference added.  Lane (i, c) holds, for group k, the
// cell of indices [k*1024/sizeof(T) + lane*N, + N), N = 16/sizeof(T).  W = 0: `last` wraps, the reads stay inside the image, the field
// mask is 0 and every field is 0.
template <typename T, typename F>
__device__ __forceinline__ void for_each_funnelled_cell(unsigned w, const char* lds, unsigned lane, F&& f)
{
    using G = WaveBlock<T>;
    constexpr int TB = G::TB;
    const unsigned c16 = (lane & 7u) * 16u;
    const typename G::word_t m = G::field_mask(w);
    unsigned bit = __umul24(G::row_base(lane >> 3), w);
    const unsigned step = G::KSTEP * w;
    const unsigned last = (w - 1u) * 128u;
    static_for<G::GROUPS>([&](auto K) {
        const unsigned word = bit >> G::LOG_TB, sh = bit & (TB - 1u);
        const unsigned a0 = word * 128u;
        const unsigned a1 = a0 + 128u < last ? a0 + 128u : last;            // the last row never reads past the end (macros.rs:156)
        const Cell<T> cur = __builtin_bit_cast(Cell<T>, *reinterpret_cast<const u32x4*>(lds + a0 + c16));
        const Cell<T> nxt = __builtin_bit_cast(Cell<T>, *reinterpret_cast<const u32x4*>(lds + a1 + c16));
        f(K, bit, G::funnel(cur, nxt, sh, m));
        bit += step;
    });
}

// verdicts[k]: bit e = element e of the lane's cell of group k -> the block's 1024-bit mask in the first 128 bytes of its image, which
// is dead once every lane holds its verdicts.  u8 / u16 write their 16 / 8 bits as they are; u32 / u64 first join 2 / 4 neighbouring
// lanes' bits into a byte (DPP quad_perm, full wave).
template <typename T>
__device__ __forceinline__ void verdicts_to_image(const uint32_t (&verdicts)[WaveBlock<T>::GROUPS], char* lds, unsigned lane)
{
    constexpr unsigned N = Elem<T>::PER_CELL;
    wave_lds_fence();                                                       // every lane holds its verdicts: the image is dead
    static_for<WaveBlock<T>::GROUPS>([&](auto K) {
        constexpr unsigned k = decltype(K)::value;
        uint32_t v = verdicts[k];
        char* at = lds + k * (128u / sizeof(T)) + lane * N / 8u;            // byte of mask bit k*1024/sizeof(T) + lane*N
        if constexpr (sizeof(T) == 1) {
            *reinterpret_cast<uint16_t*>(at) = (uint16_t)v;
        } else if constexpr (sizeof(T) == 2) {
            *reinterpret_cast<uint8_t*>(at) = (uint8_t)v;
        } else {
            v |= butterfly_partner<0>(v) << N;                              // + lane ^ 1's bits
            if constexpr (N == 2) v |= butterfly_partner<1>(v) << 4u;       // + lane ^ 2's (u64: 4 lanes per byte)
            if ((lane & (8u / N - 1u)) == 0u) *reinterpret_cast<uint8_t*>(at) = (uint8_t)v;
        }
    });
    wave_lds_fence();
}

// ONE block per call.  widths[blk], offsets[blk] and references[blk * ref_stride]: independent vector loads (z: opaque_zero), issued
// here and still in flight on return -- the kernel issues its own loads of the block behind them, then settles all of them with one wait.
template <typename T> struct BlockLoads {
    unsigned z, wv;
    uint64_t ov;
    T rv;
};
template <typename T> __device__ __forceinline__ BlockLoads<T> issue_block_loads(const WidthsArgs& a, const void* refs, uint64_t blk)
{
    BlockLoads<T> l{opaque_zero(), a.uniform_width, 0, 0};
    if (a.widths) l.wv = a.widths[blk + l.z];
    if (a.offsets) l.ov = a.offsets[blk + l.z];
    l.rv = static_cast<const T*>(refs)[blk * a.ref_stride + l.z];
    return l;
}
// the loads' values, wave-uniform, and the block's preconditions (err != 0: the block is skipped and err raised; bitpacking.rs:126
// unreachable!(), :111-113)
struct BlockMeta {
    unsigned w;
    uint64_t off, r;
    uint32_t err;
};
template <typename T> __device__ __forceinline__ BlockMeta settle_block_loads(const WidthsArgs& a, uint64_t blk, const BlockLoads<T>& l)
{
    BlockMeta m;
    m.w = (unsigned)__builtin_amdgcn_readfirstlane(l.wv);
    m.off = a.offsets ? wave_uniform_u64(l.ov) : blk * (uint64_t)(128u * m.w);
    m.r = wave_uniform_u64((uint64_t)l.rv);
    m.err = block_precondition(a, m.w, m.off, WaveBlock<T>::TB);
    return m;
}

// the w >= 1 packed rows of block `blk` at `off` -> the wavefront's LDS image, ready to be read
template <typename T>
__device__ __forceinline__ void fill_block_image(const WidthsArgs& a, uint64_t blk, uint64_t off, unsigned w, char* lds, unsigned lane)
{
    // wave-uniform descriptor over exactly this block's 128*w bytes: cells past it read as 0, no fault
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.packed) + off, 0, 128u * w, 0x00020000);
    Cell<T> no_ref;
    if (a.widths || w >= a.nt_from) packed_block_to_lds<T, RD_DMA_NT>(a, blk, rs, w, lds, lane, no_ref);   // RD_AUTO (fl_widths.hpp)
    else packed_block_to_lds<T, RD_VGPR>(a, blk, rs, w, lds, lane, no_ref);
    wave_lds_fence();
}

// SEVERAL consecutive blocks per wavefront (the narrow types), as unpack_blocks_wave_prefetched: lane j < count <= 16 holds the width,
// offset, reference and precondition bits of block first + j (the other lanes: of block `first`), judged BEFORE any packed load is issued
template <typename T> struct LaneBlocks {
    bool owner;                // lane < count
    uint64_t mine;             // the lane's block
    unsigned wv;
    uint64_t ov;
    T rv;
    uint32_t ev;
};
template <typename T>
__device__ __forceinline__ LaneBlocks<T> lane_block_loads(const WidthsArgs& a, const void* refs, uint64_t first, unsigned count, unsigned lane)
{
    LaneBlocks<T> l;
    l.owner = lane < count;
    l.mine = first + (l.owner ? lane : 0u);
    l.wv = a.uniform_width;
    if (a.widths) l.wv = a.widths[l.mine];
    l.ov = l.mine * (uint64_t)(128u * l.wv);
    if (a.offsets) l.ov = a.offsets[l.mine];
    l.rv = static_cast<const T*>(refs)[l.mine * a.ref_stride];
    l.ev = block_precondition(a, l.wv, l.ov, WaveBlock<T>::TB);
    return l;
}

// the rows of block first + j (j wave-uniform), requested by LDS-DMA into image j.  A width-0 block requests nothing: 8 * g < 0 never holds.
template <typename T>
__device__ __forceinline__ void request_block_image(const WidthsArgs& a, const LaneBlocks<T>& l, unsigned j, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)l.wv, (int)j);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.packed) + readlane_u64(l.ov, j), 0, 128u * w, 0x00020000);
    char* img = lds + j * G::BLOCK_BYTES;
    static_for<G::GROUPS>([&](auto Gi) {
        constexpr int g = decltype(Gi)::value;
        if (8u * g < w) dma_1k_to_lds<RD_DMA_NT, g * 1024>(rs, img, lane);
    });
}
// the blocks first + j, j < count, with bit j of `fetch` (wave-uniform) set, then ONE wait
template <typename T>
__device__ __forceinline__ void request_block_images(const WidthsArgs& a, const LaneBlocks<T>& l, uint64_t fetch, unsigned count, char* lds, unsigned lane)
{
    for (unsigned j = 0; j < count; ++j) {                                  // wave-uniform loop
        if ((fetch >> j) & 1u) request_block_image<T>(a, l, j, lds, lane);
    }
    wait_lds_dma();
    wave_lds_fence();
}
// the same for exactly BPW blocks, unrolled
template <typename T, unsigned BPW>
__device__ __forceinline__ void request_block_images(const WidthsArgs& a, const LaneBlocks<T>& l, uint64_t fetch, char* lds, unsigned lane)
{
    static_for<(int)BPW>([&](auto J) {
        constexpr unsigned j = decltype(J)::value;
        if ((fetch >> j) & 1u) request_block_image<T>(a, l, j, lds, lane);
    });
    wait_lds_dma();
    wave_lds_fence();
}

// The launch shapes the *_blocks_wave_static functions of select and aggregate serve (any other shape runs block by block through the
// wavefront's first image): the narrow types' shipped ones.  They keep the wavefront's BPW masks in a stash of BPW * 128 bytes of
// wave-private LDS behind the workgroup's block images.
template <typename T> __host__ __device__ inline bool static_shape(unsigned bpw, unsigned prefetch)
{
    return sizeof(T) <= 2 && prefetch != 0u && (bpw == 2u || bpw == 4u);
}
template <typename T> __device__ __forceinline__ uint32_t* wave_mask_stash(unsigned bpw)
{
    extern __shared__ __attribute__((aligned(16))) char lds_all[];
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    return reinterpret_cast<uint32_t*>(lds_all + (WG / 64) * WaveBlock<T>::BLOCK_BYTES * bpw) + wave * bpw * SELECT_MASK_WORDS;
}
// the masks of blocks first .. first + BPW - 1 (mask == nullptr: every row) into the stash, two blocks per load.  Returns, wave-uniform,
// bit j = block first + j keeps something.
template <unsigned BPW>
__device__ __forceinline__ unsigned stash_block_masks(const uint32_t* mask, uint64_t first, uint32_t* stash, unsigned lane)
{
    static_assert(BPW >= 2 && BPW <= 16 && BPW % 2 == 0, "two blocks' masks per load");
    uint32_t mw[BPW / 2];
    static_for<(int)(BPW / 2)>([&](auto I) {
        constexpr unsigned i = decltype(I)::value;
        mw[i] = ~0u;
        if (mask) mw[i] = mask[(first + 2u * i) * SELECT_MASK_WORDS + lane];   // words of blocks first + 2i (lanes 0..31) and first + 2i + 1
    });
    unsigned nonempty = 0;
    static_for<(int)(BPW / 2)>([&](auto I) {
        constexpr unsigned i = decltype(I)::value;
        stash[i * 64u + lane] = mw[i];
        const uint64_t nz = __builtin_amdgcn_ballot_w64(mw[i] != 0u);
        nonempty |= ((uint32_t)nz != 0u ? 1u : 0u) << (2u * i) | ((uint32_t)(nz >> 32) != 0u ? 2u : 0u) << (2u * i);
    });
    return nonempty;
}
// the lane's slices of block first + j's mask, back out of the stash (after the fence of request_block_images)
template <typename T>
__device__ __forceinline__ void stashed_slices(const uint32_t* stash, unsigned j, unsigned lane, uint32_t (&slice)[SelectMap<sizeof(T)>::GROUPS])
{
    using M = SelectMap<sizeof(T)>;
    static_for<(int)M::GROUPS>([&](auto K) {
        constexpr unsigned k = decltype(K)::value;
        slice[k] = M::slice(stash[j * SELECT_MASK_WORDS + M::mask_word(k, lane)], k, lane);
    });
}

// Launched with the shape of unfor_pack_widths (the C ABI passes fl_dispatch.hpp's mixed_* choices through with_policy); the tile map is
// plan_blocks', rotated for mixed-width columns as in launch_widths.  STASH: the masks' stash rides behind the workgroup's block images.
template <typename T, typename Args, void (*KERNEL)(Args), bool STASH>
hipError_t launch_block_consumer(const Args& a0, int waves, hipStream_t s)
{
    if (a0.n_blocks == 0) return hipSuccess;
    Args a = a0;
    const unsigned need = tidy_wave_blocks<T>(a.bpw, a.prefetch) + (STASH && static_shape<T>(a.bpw, a.prefetch) ? (WG / 64) * a.bpw * SELECT_MASK_WORDS * 4u : 0u);
    const unsigned grid = plan_blocks(a, a.n_blocks, a.bpw * (WG / 64), WIN_UNPACK, WaveBlock<T>::TB, a.widths != nullptr);
    const unsigned lds = occupancy_lds(waves, need);
    if (!grid || lds > 64 * 1024) return hipErrorInvalidValue;         // > 2^33 blocks; beyond the default dynamic-LDS limit
    FL_LAUNCH(KERNEL, dim3(grid), dim3(WG), lds, s, a);
    return hipGetLastError();
}

}  // namespace fl
