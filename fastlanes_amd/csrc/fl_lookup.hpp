// fl_lookup.hpp -- unfor_lookup: a dimension attribute fetched through a FoR-packed key column over the rows a selection mask keeps
// (the PROBE side of a payload join; its semi-join sibling is unfor_compare_in, fl_for_compare_in.hpp), written as a column every
// operator here consumes unchanged.  EXTENSION, defined as a composition of reference functions; all key arithmetic
// mod 2^T; U = T or uint8_t:
//     for every block b, every i in 0..1023:
//         kept = mask == nullptr or bit i of block b of `mask`
//         key  = unfor_pack::<W_b>(key block b, references[b * ref_stride])[i]                                   (ffor.rs:38-50)
//         j    = (key - key_lo) mod 2^T
//         hit  = kept and j < n_slots and (present == nullptr or bit j of present)
//         v[i] = hit ? table[j] : missing;   h[i] = hit
//     out block b      = pack::<8 * sizeof(U)>(v)        -- a permutation of v (bitpacking.rs); for U = u8 it is v itself
//     hit_mask block b = h                               -- 32 words, unpack_compare's layout
//     stats[0] += #hit;  stats[1] += #(kept and not hit)
// The window is unfor_set_build's (fl_set_decide.hpp), and with c = (reference - key_lo) the f + c of the compare kernels is j.
// A run-walking kernel (fl_block_run.hpp: the run, the look-ahead, the stats tail).  Per block, through the steps of fl_for_block.hpp:
// the route comes from fl_lookup_map.hpp (lookup_route): an empty mask and a block outside the
// window are all `missing` with no packed load and no gather, a width-0 block inside the window is one wave-uniform table read (and at
// most one `present` bit) broadcast under the mask; every other block fills its LDS image as unfor_compare_in does and funnels f + c = j
// in the lane map.  A lane's 16 table reads are all issued before the first is used, and so are its 16 bitmap words when `present` is
// given.  Two tiers, chosen once on the host (fl_lookup_map.hpp: lookup_tier):
//   * LOOKUP_LDS, n_slots * sizeof(U) <= LOOKUP_LDS_BYTES: the wavefront copies the table into LDS once and looks up with LDS reads;
//   * LOOKUP_MEM, larger tables: one vector gather load of sizeof(U) bytes per kept in-window element, default (cached) policy -- a
//     dimension table is re-read -- through a descriptor bounded to the table's bytes; an index outside the window (or a row the mask
//     drops) is given an offset past it, reads 0 and touches no memory.
// `present` is gathered through its own bounded descriptor with the cached policy in BOTH tiers (unfor_compare_in's memory tier).
// The looked-up values are written into the dead image at their PACKED FULL-WIDTH position -- U = T: the lane's own cell positions at
// w = T bits (address-row row_base(lane / 8) + k * KSTEP, the cell unpack reads there at W = T); U = u8 from a wider T: byte i of a 1-KiB
// image -- and leave as 1-KiB contiguous vector stores with the decode kernels' store policy.  Hit bits go through verdicts_to_image
// and the 128-byte store of store_range_mask, so `hit_mask` may be `mask` itself: a block's mask slices are in registers before its
// words are written, and no other wavefront touches those bytes.  Every valid block's output block (and mask words, when hit_mask is
// given) is always written.  A block that fails the mixed-width device checks raises its FL_DEVERR_* bit and is left alone.  Hits and
// misses are counted per lane (folded with wave_sum_u64, fl_block_run.hpp).
// LDS is wave-local (in-order per wave): no s_barrier.  Every global store or atomic is a vector instruction.
#pragma once
#include "fl_block_run.hpp"
#include "fl_lookup_map.hpp"

namespace fl {

// WidthsArgs::refs and ::unpacked stay nullptr: the reference is loaded with the block's metadata
struct LookupArgs {
    WidthsArgs col;
    const void* refs;              // references[b * col.ref_stride]
    const uint32_t* mask;          // [n_blocks][32]; nullptr = every row is kept (no mask is read)
    const void* table;             // U[n_slots]; never read when n_slots == 0
    const uint32_t* present;       // ceil(n_slots / 32) words; nullptr = every slot is present
    char* out;                     // [n_blocks][1024] of U, each block in full-width packed order
    uint32_t* hit_mask;            // [n_blocks][32]; nullptr = not written; may be `mask`
    uint64_t* stats;               // {hits, misses}; nullptr = not counted
    uint64_t cmp_a, cmp_s;         // the window as a ForPredicate: key_lo, n_slots - 1
    uint64_t missing;              // the value of a row that does not hit, zero-extended
    unsigned cmp_none;             // n_slots == 0
    unsigned table_bytes;          // n_slots * sizeof(U) < 2^31: the table descriptor's size
    unsigned present_bytes;        // 4 * ceil(n_slots / 32): the bitmap descriptor's size
    uint64_t run;                  // blocks of a wavefront's run; filled by the launcher
};

constexpr uint32_t LOOKUP_PAST = 0x80000000u;    // a byte offset past any table (< 2^31 bytes) and any bitmap (<= 2^29 bytes)

template <typename T, typename U, int TIER> constexpr unsigned lookup_lds()
{
    return lookup_wave_lds(WaveBlock<T>::BLOCK_BYTES, Elem<T>::BITS, (unsigned)sizeof(U), TIER == LOOKUP_LDS);
}

// table[j] (want) or 0: an LDS read of the private copy, or a bounded gather of sizeof(U) bytes
template <typename U, int TIER>
__device__ __forceinline__ U lookup_fetch(const __amdgpu_buffer_rsrc_t& ts, const char* tab, uint32_t j, bool want)
{
    if constexpr (TIER == LOOKUP_LDS) {
        return *reinterpret_cast<const U*>(tab + (want ? j * (uint32_t)sizeof(U) : 0u));
    } else {
        const uint32_t at = want ? j * (uint32_t)sizeof(U) : LOOKUP_PAST;
        if constexpr (sizeof(U) == 1) return (U)__builtin_amdgcn_raw_buffer_load_b8(ts, at, 0, 0);
        else if constexpr (sizeof(U) == 2) return (U)__builtin_amdgcn_raw_buffer_load_b16(ts, at, 0, 0);
        else if constexpr (sizeof(U) == 4) return (U)__builtin_amdgcn_raw_buffer_load_b32(ts, at, 0, 0);
        else return __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(ts, at, 0, 0));
    }
}

// a block's loads, issued and possibly still in flight
template <typename T> struct LookupLoads {
    BlockLoads<T> m;
    uint32_t slice[SelectMap<sizeof(T)>::GROUPS];
};
template <typename T> __device__ __forceinline__ LookupLoads<T> lookup_issue(const LookupArgs& a, uint64_t blk, unsigned lane)
{
    LookupLoads<T> p;
    p.m = issue_block_loads<T>(a.col, a.refs, blk);
    block_mask_slices<T>(a.mask, blk, lane, p.slice);
    return p;
}

// block `blk`'s 128 mask bytes from lanes 0 .. 7, 16 bytes each (store_range_mask's store); every other lane's lands past the descriptor
__device__ __forceinline__ void lookup_store_mask(const LookupArgs& a, uint64_t blk, u32x4 v, unsigned lane)
{
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(a.hit_mask) + blk * 128u, 0, 128u, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, lane < 8u ? lane * 16u : 128u, 0, STORE_AUX);
}

// a block that hits nowhere: `missing` in every position (a splat is its own permutation), no hit bit
template <typename T, typename U> __device__ __forceinline__ void lookup_store_missing(const LookupArgs& a, uint64_t blk, unsigned lane)
{
    constexpr unsigned OUT_BYTES = 1024u * sizeof(U);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.out + blk * OUT_BYTES, 0, OUT_BYTES, 0x00020000);
    const u32x4 v = __builtin_bit_cast(u32x4, Cell<U>::splat((U)a.missing));
    static_for<(int)sizeof(U)>([&](auto K) { __builtin_amdgcn_raw_buffer_store_b128(v, rs, lane * 16u + decltype(K)::value * 1024u, 0, STORE_AUX); });
    if (a.hit_mask) lookup_store_mask(a, blk, u32x4{0u, 0u, 0u, 0u}, lane);
}

// The lane's values val[k * N + e] and hit bits (bit e of hits[k]) of element e of its cell of group k -> the block's output and mask.
// The image is dead: the hit bits are gathered in its first 128 bytes and stored, then the values are written at their packed
// full-width position and leave as 1-KiB contiguous stores.
template <typename T, typename U>
__device__ __forceinline__ void lookup_emit(const LookupArgs& a, uint64_t blk, char* lds, unsigned lane, const U (&val)[16],
                                            const uint32_t (&hits)[WaveBlock<T>::GROUPS])
{
    using G = WaveBlock<T>;
    constexpr int N = Elem<T>::PER_CELL, GROUPS = G::GROUPS;
    constexpr unsigned OUT_BYTES = 1024u * sizeof(U);
    static_assert(GROUPS * N == 16, "16 elements per lane whatever the type");
    if (a.hit_mask) {
        verdicts_to_image<T>(hits, lds, lane);
        lookup_store_mask(a, blk, *reinterpret_cast<const u32x4*>(lds + (lane & 7u) * 16u), lane);
    }
    wave_lds_fence();                                                       // every lane holds its values: the image is dead
    if constexpr (sizeof(U) == sizeof(T)) {
        // pack::<T>(v): address-row p of a W = T block holds logical row p's cells; the lane's cell of group k is that of unpack at W = T
        const unsigned c16 = (lane & 7u) * 16u, rb = G::row_base(lane >> 3);
        static_for<GROUPS>([&](auto K) {
            constexpr int k = decltype(K)::value;
            Cell<T> cell = Cell<T>::zero();
            static_for<N>([&](auto E) { cell_or<T>(cell, decltype(E)::value, (uint64_t)val[k * N + decltype(E)::value]); });
            *reinterpret_cast<u32x4*>(lds + (rb + (unsigned)(k * G::KSTEP)) * 128u + c16) = __builtin_bit_cast(u32x4, cell);
        });
    } else {
        // pack::<8>(v) is v: the lane's N bytes of group k at byte k * (1024 / sizeof(T)) + lane * N of a 1-KiB image
        static_assert(sizeof(U) == 1 && sizeof(T) > 1, "a u8 payload from a wider key");
        static_for<GROUPS>([&](auto K) {
            constexpr int k = decltype(K)::value;
            char* at = lds + k * (1024 / (int)sizeof(T)) + lane * N;
            uint32_t w[2] = {0u, 0u};
            static_for<N>([&](auto E) {
                constexpr int e = decltype(E)::value;
                w[e / 4] |= (uint32_t)val[k * N + e] << (8 * (e % 4));
            });
            if constexpr (N == 8) *reinterpret_cast<uint64_t*>(at) = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
            else if constexpr (N == 4) *reinterpret_cast<uint32_t*>(at) = w[0];
            else *reinterpret_cast<uint16_t*>(at) = (uint16_t)w[0];
        });
    }
    wave_lds_fence();
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.out + blk * OUT_BYTES, 0, OUT_BYTES, 0x00020000);
    static_for<(int)sizeof(U)>([&](auto K) {
        constexpr unsigned g = decltype(K)::value;
        __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(lds + g * 1024u + lane * 16u), rs, g * 1024u + lane * 16u, 0, STORE_AUX);
    });
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

// one block whose loads were issued by lookup_issue.  lds: [image | private table (LOOKUP_LDS)]; hit / miss: the lane's counters
template <typename T, typename U, int TIER>
__device__ __forceinline__ void lookup_block(const LookupArgs& a, uint64_t blk, const LookupLoads<T>& p, char* lds, const char* tab,
                                             const __amdgpu_buffer_rsrc_t& ts, const __amdgpu_buffer_rsrc_t& ps, unsigned lane, uint64_t& hit,
                                             uint64_t& miss)
{
    using G = WaveBlock<T>;
    using M = SelectMap<sizeof(T)>;
    constexpr int N = Elem<T>::PER_CELL, GROUPS = G::GROUPS;
    static_assert(M::GROUPS == (unsigned)GROUPS && M::N == (unsigned)N, "fl_select_map.hpp follows fl_widths.hpp's lane map");
    const BlockMeta m = settle_block_loads<T>(a.col, blk, p.m);
    uint32_t any = 0, kept = 0;
    static_for<GROUPS>([&](auto K) {
        any |= p.slice[decltype(K)::value];
        kept += (uint32_t)__builtin_popcount(p.slice[decltype(K)::value]);  // the lane's kept rows
    });
    const bool empty = __builtin_amdgcn_ballot_w64(any != 0u) == 0ull;
    if (m.err) raise_device_error(a.col.err_flag, m.err, lane);
    uint64_t c;
    const LookupRoute route = lookup_route(G::TB, ForPredicate{a.cmp_a, a.cmp_s, a.cmp_none != 0u}, empty, m.err == 0u, m.r, m.w, c);
    if (route == LOOKUP_SKIP) return;
    if (route == LOOKUP_MISSING) {
        lookup_store_missing<T, U>(a, blk, lane);
        miss += kept;
        return;
    }
    const U none = (U)a.missing;
    U val[16];
    uint32_t hits[GROUPS];
    if (route == LOOKUP_ONE_SLOT) {                                         // width 0 inside the window: slot c, c wave-uniform
        uint32_t word = ~0u;
        if (a.present) word = (uint32_t)__builtin_amdgcn_readfirstlane((int)__builtin_amdgcn_raw_buffer_load_b32(ps, (uint32_t)(c >> 5) << 2, 0, 0));
        if (((word >> (c & 31u)) & 1u) == 0u) {                             // the slot is absent: as a block outside the window
            lookup_store_missing<T, U>(a, blk, lane);
            miss += kept;
            return;
        }
        const U v = lookup_fetch<U, TIER>(ts, tab, (uint32_t)c, true);      // one address for the wavefront
        static_for<GROUPS>([&](auto K) {
            constexpr int k = decltype(K)::value;
            hits[k] = p.slice[k];
            static_for<N>([&](auto E) { val[k * N + decltype(E)::value] = ((p.slice[k] >> decltype(E)::value) & 1u) != 0u ? v : none; });
        });
        hit += kept;
        lookup_emit<T, U>(a, blk, lds, lane, val, hits);
        return;
    }
    fill_block_image<T>(a.col, blk, m.off, m.w, lds, lane);
    const Cell<T> cc = Cell<T>::splat((T)c);
    const T s = (T)a.cmp_s;
    uint32_t at[16], word[16];
    uint32_t want = 0;                                                      // bit i: element i is kept and inside the window
    for_each_funnelled_cell<T>(m.w, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) {
        const Cell<T> j = cell.add(cc);                                     // (f + c) mod 2^T per element: the slot
        const uint32_t sl = p.slice[decltype(K)::value];
        static_for<N>([&](auto E) {
            constexpr int i = decltype(K)::value * N + decltype(E)::value;
            const T x = (T)cell_get<T>(j, decltype(E)::value);
            const bool in = ((sl >> decltype(E)::value) & 1u) != 0u && x <= s;
            at[i] = (uint32_t)x;                                            // a slot inside the window is < 2^32
            want |= (in ? 1u : 0u) << i;
        });
    });
    // the lane's 16 table reads, then its 16 bitmap words: all requested before the first is looked at
    static_for<16>([&](auto I) {
        constexpr int i = decltype(I)::value;
        val[i] = lookup_fetch<U, TIER>(ts, tab, at[i], ((want >> i) & 1u) != 0u);
    });
    if (a.present) {
        static_for<16>([&](auto I) {
            constexpr int i = decltype(I)::value;
            word[i] = __builtin_amdgcn_raw_buffer_load_b32(ps, ((want >> i) & 1u) != 0u ? (at[i] >> 5) << 2 : LOOKUP_PAST, 0, 0);
        });
        static_for<16>([&](auto I) {
            constexpr int i = decltype(I)::value;
            want &= ~((((word[i] >> (at[i] & 31u)) & 1u) ^ 1u) << i);       // a clear bit: no hit (a word past the bitmap reads 0)
        });
    }
    static_for<GROUPS>([&](auto K) {
        constexpr int k = decltype(K)::value;
        hits[k] = (want >> (k * N)) & ((1u << N) - 1u);
        static_for<N>([&](auto E) {
            constexpr int i = k * N + decltype(E)::value;
            val[i] = ((want >> i) & 1u) != 0u ? val[i] : none;
        });
    });
    const uint32_t n_hit = (uint32_t)__builtin_popcount(want);
    hit += n_hit;
    miss += kept - n_hit;
    lookup_emit<T, U>(a, blk, lds, lane, val, hits);
}

// Workgroup (= wavefront) g owns blocks [g * run, (g + 1) * run) of the column; one that owns none returns before it touches LDS.
template <typename T, typename U, int TIER>
__global__ __launch_bounds__(64) void k_unfor_lookup(LookupArgs a)
{
    using G = WaveBlock<T>;
    extern __shared__ __attribute__((aligned(16))) char lds_all[];
    const unsigned lane = threadIdx.x;
    const uint64_t n = a.col.n_blocks;
    const uint64_t first = (uint64_t)blockIdx.x * a.run;
    if (first >= n) return;
    const uint64_t end = n - first < a.run ? n : first + a.run;
    char* tab = lds_all + G::BLOCK_BYTES;
    const __amdgpu_buffer_rsrc_t ts = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.table), 0, a.table_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ps = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(a.present), 0, a.present_bytes, 0x00020000);
    LookupLoads<T> cur = lookup_issue<T>(a, first, lane);
    if constexpr (TIER == LOOKUP_LDS) {
        // the table's whole words, then its last 1 .. 3 bytes: nothing past table_bytes is read (table_bytes <= the private copy's)
        const unsigned words = a.table_bytes >> 2, tail = a.table_bytes & 3u;
        for (unsigned i = lane; i < words; i += 64u) reinterpret_cast<uint32_t*>(tab)[i] = static_cast<const uint32_t*>(a.table)[i];
        if (lane < tail) tab[words * 4u + lane] = static_cast<const char*>(a.table)[words * 4u + lane];
        wave_lds_fence();
    }
    uint64_t hit = 0, miss = 0;
    for (uint64_t blk = first; blk < end; ++blk) {                          // wave-uniform loop
        const uint64_t ahead = blk + 1 < end ? blk + 1 : blk;               // the last block asks for itself again: straight-line code
        const LookupLoads<T> nxt = lookup_issue<T>(a, ahead, lane);
        lookup_block<T, U, TIER>(a, blk, cur, lds_all, tab, ts, ps, lane, hit, miss);
        cur = nxt;
    }
    if (a.stats) {
        hit = wave_sum_u64(hit);
        miss = wave_sum_u64(miss);
        if (lane == 0u && hit != 0ull) __hip_atomic_fetch_add(a.stats, hit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0u && miss != 0ull) __hip_atomic_fetch_add(a.stats + 1, miss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <typename T, typename U, int TIER>
hipError_t launch_lookup(const LookupArgs& a, int waves, hipStream_t s)
{
    return launch_group_runs<k_unfor_lookup<T, U, TIER>, lookup_lds<T, U, TIER>()>(a, a.col.n_blocks, a.col.bpw, waves, s);
}

typedef hipError_t (*lookup_launch_t)(const LookupArgs&, int waves, hipStream_t);
// payload_bytes: sizeof(T) or 1; nullptr for a pair that does not exist (u8 has no u8 twin, and no memory tier)
template <typename T> lookup_launch_t lookup_launcher(unsigned payload_bytes, int tier);

}  // namespace fl
