// fl_for_compare.hpp -- unfor_compare: a selection mask straight from a FoR-packed column, uniform or mixed width.
// EXTENSION, defined as a composition of reference functions:
//     bit i of mask[b*32 .. b*32+32) = (unfor_pack::<W_b>(block b, references[b * ref_stride])[i] <op> constant)
// (ffor.rs:38-50; i in the unpacked index order, LSB first, 32 words per block: unpack_compare's layout, fl_consume.hpp).
// The wave-per-block machinery of fl_widths.hpp (one wavefront per block, runtime width, the LDS image, WaveBlock::funnel) with
// the predicate arithmetic of fl_for_decide.hpp:
//   * a block's width, offset AND reference arrive together (three vector loads, one wait -- block_ref loads the reference
//     behind the data instead), its preconditions are checked (block_precondition: a failing block is skipped and its mask
//     words are left untouched, as unpack_widths leaves its output), then the block is decided;
//   * a DECIDED block (its fields' cyclic range lies inside, or outside, the predicate's interval) issues no packed load and
//     writes its 128-byte mask as all ones or all zeros;
//   * an undecided block fills its LDS image as unpack_widths does, and lane (i, c) funnels its cell of each 1-KiB group --
//     16/sizeof(T) consecutive indices -- adds c and compares with s (SWAR for u8 / u16, v_cmp for u32 / u64: row_predicate_bits
//     with W = T); the verdict bits are gathered into the first 128 bytes of the (by then dead) image and leave as ONE coalesced
//     128-byte store (lanes 0..7, 16 bytes each).
// LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_widths.hpp"
#include "fl_consume.hpp"
#include "fl_for_decide.hpp"

namespace fl {

// WidthsArgs::refs and ::unpacked stay nullptr: the reference is loaded with the block's metadata, the output is the mask
struct ForCompareArgs : WidthsArgs {
    char* mask;                // [n_blocks][128 bytes]
    const void* cmp_refs;      // references[b * ref_stride]
    uint64_t cmp_a, cmp_s;     // the predicate: (v - cmp_a) mod 2^T <= cmp_s  (fl_for_decide.hpp, reduced on the host)
    unsigned cmp_none;         // 1: no value satisfies it
};

__device__ __forceinline__ ForPredicate predicate_of(const ForCompareArgs& a) { return ForPredicate{a.cmp_a, a.cmp_s, a.cmp_none != 0u}; }

// block `blk`'s 128-byte mask: lanes 0..7 store 16 bytes each, the descriptor drops the other lanes' stores
__device__ __forceinline__ void store_block_mask(const ForCompareArgs& a, uint64_t blk, u32x4 v, unsigned lane)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.mask + blk * 128u, 0, 128u, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, lane * 16u, 0, STORE_AUX);
}
__device__ __forceinline__ void store_decided_mask(const ForCompareArgs& a, uint64_t blk, int verdict, unsigned lane)
{
    const uint32_t m = verdict == FOR_CMP_ALL ? ~0u : 0u;
    store_block_mask(a, blk, u32x4{m, m, m, m}, lane);
}

// The LDS image of an undecided block (1 <= w <= T rows) -> its mask.  Lane (i, c) holds, for 1-KiB group k, the cell of indices
// [k*1024/sizeof(T) + lane*N, + N), N = 16/sizeof(T): bits at the same positions of the block's 1024-bit mask.  u8 / u16 write
// their 16 / 8 bits as they are; u32 / u64 first join 2 / 4 neighbouring lanes' bits into a byte (DPP quad_perm, full wave).
template <typename T>
__device__ __forceinline__ void compare_lds_image(const ForCompareArgs& a, uint64_t blk, unsigned w, char* lds, unsigned lane, T c)
{
    using G = WaveBlock<T>;
    constexpr int TB = G::TB;
    constexpr unsigned N = Elem<T>::PER_CELL;
    const unsigned c16 = (lane & 7u) * 16u;
    const typename G::word_t m = G::field_mask(w);
    unsigned bit = __umul24(G::row_base(lane >> 3), w);
    const unsigned step = G::KSTEP * w;
    const unsigned last = (w - 1u) * 128u;
    const Cell<T> cc = Cell<T>::splat(c);
    const T s = (T)a.cmp_s;
    uint32_t verdicts[G::GROUPS];
    static_for<G::GROUPS>([&](auto K) {
        const unsigned word = bit >> G::LOG_TB, sh = bit & (TB - 1u);
        const unsigned a0 = word * 128u;
        const unsigned a1 = a0 + 128u < last ? a0 + 128u : last;            // the last row never reads past the end (macros.rs:156)
        const Cell<T> cur = __builtin_bit_cast(Cell<T>, *reinterpret_cast<const u32x4*>(lds + a0 + c16));
        const Cell<T> nxt = __builtin_bit_cast(Cell<T>, *reinterpret_cast<const u32x4*>(lds + a1 + c16));
        // ((f + c) mod 2^T) <= s per element: bit e = element e of the cell
        verdicts[decltype(K)::value] = row_predicate_bits<T, TB, false>(G::funnel(cur, nxt, sh, m).add(cc), s);
        bit += step;
    });
    wave_lds_fence();                                                       // every lane holds its verdicts: the image is dead
    static_for<G::GROUPS>([&](auto K) {
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
    store_block_mask(a, blk, *reinterpret_cast<const u32x4*>(lds + lane * 16u), lane);
}

// one block per call: metadata + reference, checks, verdict, and only for an undecided block the packed rows
template <typename T>
__device__ __forceinline__ void compare_block_wave(const ForCompareArgs& a, uint64_t blk, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    constexpr int TB = G::TB;
    // widths[blk], offsets[blk] and the reference: independent vector loads in flight together, one wait, then wave-uniform
    const unsigned z = opaque_zero();
    unsigned wv = a.uniform_width;
    uint64_t ov = 0;
    if (a.widths) wv = a.widths[blk + z];
    if (a.offsets) ov = a.offsets[blk + z];
    const T rv = static_cast<const T*>(a.cmp_refs)[blk * a.ref_stride + z];
    const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(wv);
    const uint64_t off = a.offsets ? wave_uniform_u64(ov) : blk * (uint64_t)(128u * w);
    const uint64_t r = wave_uniform_u64((uint64_t)rv);
    if (const uint32_t e = block_precondition(a, w, off, TB)) {            // bitpacking.rs:126 unreachable!(), :111-113
        raise_device_error(a.err_flag, e, lane);
        return;
    }
    uint64_t c;
    const int verdict = for_compare_decide(TB, predicate_of(a), r, w, c);
    if (verdict != FOR_CMP_EACH) {                                          // (W = 0 always ends here)
        store_decided_mask(a, blk, verdict, lane);
        return;
    }
    // wave-uniform descriptor over exactly this block's 128*w bytes: cells past it read as 0, no fault
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.packed) + off, 0, 128u * w, 0x00020000);
    Cell<T> no_ref;
    if (a.widths || w >= a.nt_from) packed_block_to_lds<T, RD_DMA_NT>(a, blk, rs, w, lds, lane, no_ref);   // RD_AUTO (fl_widths.hpp)
    else packed_block_to_lds<T, RD_VGPR>(a, blk, rs, w, lds, lane, no_ref);
    wave_lds_fence();
    compare_lds_image<T>(a, blk, w, lds, lane, (T)c);
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, unsigned j)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j);
}

// Several consecutive blocks per wavefront (the narrow types), as unpack_blocks_wave_prefetched: lane j judges block first + j --
// metadata, reference, preconditions and verdict -- BEFORE any packed load is issued; only the undecided blocks' rows are then
// requested by LDS-DMA, one image per block, one wait, and the blocks are answered back to back.
template <typename T>
__device__ __forceinline__ void compare_blocks_wave_prefetched(const ForCompareArgs& a, uint64_t first, unsigned count, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    constexpr int TB = G::TB;
    const bool owner = lane < count;                          // count <= 16 <= 64 lanes
    const uint64_t mine = first + (owner ? lane : 0u);
    unsigned wv = a.uniform_width;
    if (a.widths) wv = a.widths[mine];
    uint64_t ov = mine * (uint64_t)(128u * wv);
    if (a.offsets) ov = a.offsets[mine];
    const T rv = static_cast<const T*>(a.cmp_refs)[mine * a.ref_stride];
    const uint32_t ev = block_precondition(a, wv, ov, TB);
    uint64_t cv = 0;
    const int vv = ev ? (int)FOR_CMP_EACH : for_compare_decide(TB, predicate_of(a), rv, wv, cv);
    const uint64_t fetch = __builtin_amdgcn_ballot_w64(owner && ev == 0u && vv == FOR_CMP_EACH);
    for (unsigned j = 0; j < count; ++j) {                    // wave-uniform loop
        if (!((fetch >> j) & 1u)) continue;
        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)wv, (int)j);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.packed) + readlane_u64(ov, j), 0, 128u * w, 0x00020000);
        char* img = lds + j * G::BLOCK_BYTES;
        static_for<G::GROUPS>([&](auto Gi) {
            constexpr int g = decltype(Gi)::value;
            if (8u * g < w) dma_1k_to_lds<RD_DMA_NT, g * 1024>(rs, img, lane);
        });
    }
    wait_lds_dma();
    wave_lds_fence();
    for (unsigned j = 0; j < count; ++j) {
        const uint64_t blk = first + j;
        if (const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)ev, (int)j)) {   // bitpacking.rs:126 unreachable!(), :111-113
            raise_device_error(a.err_flag, e, lane);
            continue;
        }
        const int verdict = __builtin_amdgcn_readlane(vv, (int)j);
        if (verdict != FOR_CMP_EACH) {
            store_decided_mask(a, blk, verdict, lane);
            continue;
        }
        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)wv, (int)j);
        compare_lds_image<T>(a, blk, w, lds + j * G::BLOCK_BYTES, lane, (T)readlane_u64(cv, j));
    }
}

template <typename T>
__global__ __launch_bounds__(WG) void k_unfor_compare(ForCompareArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        if (a.prefetch && count > 1) {
            compare_blocks_wave_prefetched<T>(a, first, count, lds, lane);
            return;
        }
        for (unsigned j = 0; j < count; ++j) compare_block_wave<T>(a, first + j, lds, lane);
    });
}

// Launched with the shape of unfor_pack_widths (the C ABI passes fl_dispatch.hpp's mixed_* choices through with_policy); the
// tile map is plan_blocks', rotated for mixed-width columns as in launch_widths.
typedef hipError_t (*for_compare_launch_t)(const ForCompareArgs&, int waves, hipStream_t);
template <typename T> hipError_t launch_unfor_compare(const ForCompareArgs& a0, int waves, hipStream_t s)
{
    if (a0.n_blocks == 0) return hipSuccess;
    ForCompareArgs a = a0;
    const unsigned need = tidy_wave_blocks<T>(a.bpw, a.prefetch);
    const unsigned grid = plan_blocks(a, a.n_blocks, a.bpw * (WG / 64), WIN_UNPACK, WaveBlock<T>::TB, a.widths != nullptr);
    const unsigned lds = occupancy_lds(waves, need);
    if (!grid || lds > 64 * 1024) return hipErrorInvalidValue;         // > 2^33 blocks; beyond the default dynamic-LDS limit
    FL_LAUNCH((k_unfor_compare<T>), dim3(grid), dim3(WG), lds, s, a);
    return hipGetLastError();
}
template <typename T> for_compare_launch_t for_compare_launcher();

}  // namespace fl
