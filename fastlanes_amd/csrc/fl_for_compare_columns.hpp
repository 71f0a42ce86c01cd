// fl_for_compare_columns.hpp -- unfor_compare_columns: `WHERE a <op> b` between two FoR-packed columns of the same element type and
// block count, both uniform width (possibly different widths) or both mixed width, chained through the mask so far.
// EXTENSION, defined as a composition of reference functions; all arithmetic mod 2^T:
//     va = unfor_pack::<WA_b>(a block b, a_references[b * a_ref_stride])[i]       vb likewise from column b        (ffor.rs:38-50)
//     hit[b][i] = ((va + bias) mod 2^T) <op> ((vb + bias) mod 2^T)               unsigned; bias = is_signed ? 2^(T-1) : 0
//     NEW: mask[b] = hit[b]      AND: mask[b] = mask_in[b] & hit[b]      OR: mask[b] = mask_in[b] | hit[b]
// (the masks in unpack_compare's layout, 32 words per block).  The host reduces the six ops to one base relation (x < y or x == y),
// "swap the columns" (done there: the kernel's column a is the base relation's left side) and "invert" (fl_columns_decide.hpp).
// One wavefront per block in the launch shape of unfor_pack_widths, through the steps of fl_for_block.hpp and the mask steps of
// fl_for_compare_range.hpp:
//   * both columns' width, offset and reference and the block's 128 bytes of mask_in arrive together (independent vector loads,
//     one wait); the bias is folded into the two references there; both columns' preconditions are checked: a block that fails
//     either raises its bits, keeps its mask words and reads neither column;
//   * a block is answered WITHOUT a packed load of either column when its incoming mask has closed it (AND over all-zero, OR over
//     all-ones: range_mask_live's one ballot) or when columns_decide_base decides it (both widths 0 always end here);
//   * otherwise only the columns of width >= 1 are fetched, both under ONE wait: column a's rows by LDS-DMA into the wavefront's
//     image, column b's rows into staging registers.  ONE image serves both columns -- two u64 images for each of a workgroup's four
//     wavefronts are the whole 64 KiB launch_block_consumer allows, and one image keeps the launch shape, the LDS request and the
//     residency of unfor_compare_range for every type: lane (i, c) funnels its cell of every 1-KiB group of column a and keeps the
//     16 values in registers (4 / 8 / 16 / 32 VGPRs for u8 / u16 / u32 / u64), the staged rows of column b then overwrite the dead
//     image and are funnelled in the same lane map, so the join costs nothing: per element two adds and one compare (SWAR for
//     u8 / u16: the verdict lands in each element's top bit and squeeze_bit gathers them);
//   * the verdict bits are gathered by verdicts_to_image, combined with the lane's incoming 16 bytes and leave as one coalesced
//     128-byte store (store_range_mask).
// Every valid block's 128 bytes are always written.  `mask` may be `mask_in` itself: a wavefront reads a block's incoming mask before
// it stores that block, and no other wavefront touches those bytes.  Every launch shape for_each_block_of_wave hands out is served
// block by block through the wavefront's first image; a several-blocks-in-flight form for the narrow types is an open end.
// Out of scope: columns of different element types, arithmetic inside the predicate (fl_aggregate_columns.hpp aggregates a o b), Delta columns, the host tier.
// LDS is wave-local (in-order per wave): no s_barrier.  Every store is a vector store.
#pragma once
#include "fl_for_compare_range.hpp"
#include "fl_columns_decide.hpp"
#include "fl_block_run.hpp"

namespace fl {

// The WidthsArgs base is column a (it carries the launch shape and the tile map), cmp_refs its references; cmp_a / cmp_s / cmp_none
// are unused.  Both columns have the same n_blocks and the same err_flag.
struct ForColumnsArgs : ForRangeArgs {
    WidthsArgs b;              // column b
    const void* b_refs;        // b_references[blk * b.ref_stride]
    uint64_t bias;             // 2^(T-1) for a signed comparison, else 0
    unsigned is_eq;            // base relation: 1 x == y, 0 x < y  (x from column a, y from column b)
    unsigned invert;           // 1: the answer is the complement
};

// bit e = (element e of x) <base relation> (element e of y), e < PER_CELL; the bits above are 0
template <typename T>
__device__ __forceinline__ uint32_t columns_cell_bits(const Cell<T>& x, const Cell<T>& y, bool is_eq)
{
    constexpr int N = Elem<T>::PER_CELL;
    if constexpr (sizeof(T) >= 4) {
        uint32_t bits = 0;
        static_for<N>([&](auto E) {
            constexpr int e = decltype(E)::value;
            const T p = (T)cell_get<T>(x, e), q = (T)cell_get<T>(y, e);
            bits |= (uint32_t)(is_eq ? p == q : p < q) << e;
        });
        return bits;
    } else {
        // SWAR: the verdict of an element in its top bit.  x == y: the difference's bits, ORed down, are all clear.  x < y: the
        // borrow out of x - y, (~x & y) | ((~x | y) & (x - y)).
        constexpr uint32_t H = sizeof(T) == 2 ? 0x80008000u : 0x80808080u;
        constexpr uint32_t L = ~H;
        const Cell<T> d = x.sub(y);
        uint32_t p[4];
        for (int i = 0; i < 4; ++i) {
            const uint32_t xi = x.x[i], yi = y.x[i], q = xi ^ yi;
            p[i] = is_eq ? ~(((q & L) + L) | q) : ((~xi & yi) | ((~xi | yi) & d.x[i]));
        }
        return squeeze_bit<T, (int)(sizeof(T) * 8) - 1>(p);
    }
}

// one block per call: both columns' metadata and references and the incoming mask in flight together; only an open block requests
// packed rows, and only of the columns that have any
template <typename T>
__device__ __forceinline__ void columns_block_wave(const ForColumnsArgs& a, uint64_t blk, char* lds, unsigned lane)
{
    using G = WaveBlock<T>;
    constexpr unsigned N = Elem<T>::PER_CELL;
    const BlockLoads<T> la = issue_block_loads<T>(a, a.cmp_refs, blk);
    const BlockLoads<T> lb = issue_block_loads<T>(a.b, a.b_refs, blk);
    u32x4 in = {0u, 0u, 0u, 0u};
    if (a.combine != MASK_NEW) {
        // exactly this block's 128 bytes: lanes 8..63 read past the descriptor, which returns 0 and touches no memory
        const __amdgpu_buffer_rsrc_t ms = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.mask_in) + blk * 128u, 0, 128u, 0x00020000);
        in = __builtin_amdgcn_raw_buffer_load_b128(ms, lane * 16u, 0, 0);
    }
    const BlockMeta ma = settle_block_loads<T>(a, blk, la);
    const BlockMeta mb = settle_block_loads<T>(a.b, blk, lb);
    if (const uint32_t err = ma.err | mb.err) {
        raise_device_error(a.err_flag, err, lane);
        return;
    }
    if (__builtin_amdgcn_ballot_w64(lane < 8u && range_mask_live(a.combine, in)) == 0ull) {
        store_range_mask(a, blk, in, lane, 0u);                             // AND of nothing, OR of everything: mask_in is the answer
        return;
    }
    const uint64_t ra = ma.r ^ a.bias, rb = mb.r ^ a.bias;                  // + 2^(T-1) mod 2^T: the order domain
    const int base = columns_decide_base(G::TB, a.is_eq != 0u, ra, ma.w, rb, mb.w);
    if (base != FOR_CMP_EACH) {                                             // (both widths 0 always end here)
        store_decided_range(a, blk, a.invert ? columns_invert_verdict(base) : base, in, lane, 0u);
        return;
    }
    // wave-uniform descriptors over exactly each block's 128 * w bytes (a width-0 side: none, nothing is requested of it)
    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.packed) + ma.off, 0, 128u * ma.w, 0x00020000);
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.b.packed) + mb.off, 0, 128u * mb.w, 0x00020000);
    const StagedRows<T> pk = request_image_and_staged<T>(ars, ma.w, brs, mb.w, lds, lane);
    wait_lds_dma();
    wave_lds_fence();
    // column a: the lane's 16 values into registers (W = 0: every field is 0, the value is the reference)
    Cell<T> va[G::GROUPS];
    const Cell<T> ca = Cell<T>::splat((T)ra);
    for_each_funnelled_cell<T>(ma.w, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) { va[decltype(K)::value] = cell.add(ca); });
    staged_to_image<T>(pk, mb.w, lds, lane);
    // column b through the same lane map, judged against the kept values
    uint32_t verdicts[G::GROUPS];
    const Cell<T> cb = Cell<T>::splat((T)rb);
    const uint32_t flip = a.invert ? (1u << N) - 1u : 0u;
    const bool is_eq = a.is_eq != 0u;
    for_each_funnelled_cell<T>(mb.w, lds, lane, [&](auto K, unsigned, const Cell<T>& cell) {
        constexpr int k = decltype(K)::value;
        verdicts[k] = columns_cell_bits<T>(va[k], cell.add(cb), is_eq) ^ flip;
    });
    verdicts_to_image<T>(verdicts, lds, lane);
    store_range_mask(a, blk, range_combine(a.combine, in, *reinterpret_cast<const u32x4*>(lds + (lane & 7u) * 16u)), lane, 0u);
    wave_lds_fence();                                                       // the image is reused by the wavefront's next block
}

template <typename T>
__global__ __launch_bounds__(WG) void k_unfor_compare_columns(ForColumnsArgs a)
{
    for_each_block_of_wave<T>(a, [&](uint64_t first, unsigned count, char* lds, unsigned lane) {
        for (unsigned j = 0; j < count; ++j) columns_block_wave<T>(a, first + j, lds, lane);
    });
}

typedef hipError_t (*for_columns_launch_t)(const ForColumnsArgs&, int waves, hipStream_t);   // launch_block_consumer (fl_for_block.hpp)
template <typename T> for_columns_launch_t for_columns_launcher();

}  // namespace fl
