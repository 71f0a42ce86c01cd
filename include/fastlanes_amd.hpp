// fastlanes_amd.hpp -- C++ host-side mirror of the reference's codec traits over the
// C ABI (include/fastlanes_amd.h).  The reference is compiled Rust; with no Rust
// toolchain in the build image this header plays the role of the `impl BitPacking
// for u32 { .. }` shim (INTEGRATION.md shows the Rust form): same method names,
// argument meaning and error behaviour.
//
//   reference (Rust)                                    here (C++)
//   <T as BitPacking>::pack::<W>(&in, &mut out)         fastlanes::BitPacking<T>::pack<W>(in, out)
//   <T as BitPacking>::unchecked_pack(w, in, out)       fastlanes::BitPacking<T>::unchecked_pack(w, in, n_in, out, n_out)
//   <T as FoR>::for_pack::<W>(&in, r, &mut out)         fastlanes::FoR<T>::for_pack<W>(in, r, out)
//   <T as Delta>::undelta_pack::<W>(&in, &base, &mut o) fastlanes::Delta<T>::undelta_pack<W>(in, base, out)
//   <T as Transpose>::transpose(&in, &mut out)          fastlanes::Transpose<T>::transpose(in, out)
//
// Fixed-size array references enforce the sizes the Rust types enforce
// (bitpacking.rs:19,33); `W <= T` is a static_assert (bitpacking.rs:8-13).
// The `unchecked_` forms take slices (pointer + length) and, like the reference's
// debug_asserts (bitpacking.rs:78-80), check lengths -- here always.  Where the
// reference panics (width > T: bitpacking.rs:93; index >= 1024: :152) this throws
// fastlanes::Error.  Every call runs the gfx950 kernels (host slices are staged
// through HBM); there is no CPU implementation.  `*_device` members are the batched,
// device-resident form of the same methods (n_blocks contiguous blocks, async).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "fastlanes_amd.h"

namespace fastlanes {

constexpr std::size_t FL_ORDER[8] = {0, 4, 2, 6, 1, 5, 3, 7};   // lib.rs:22

struct Error : std::runtime_error {
    int status;
    Error(int st, const char* where)
        : std::runtime_error(std::string(where) + ": " + fl_status_string(st)), status(st) {}
};

namespace detail {
inline void check(int st, const char* where) { if (st != FL_OK) throw Error(st, where); }

template <typename T> struct Abi;
#define FASTLANES_ABI(T, S)                                                                          \
    template <> struct Abi<T> {                                                                      \
        static constexpr auto pack = fl_##S##_pack;                                                  \
        static constexpr auto unpack = fl_##S##_unpack;                                              \
        static constexpr auto unpack_single = fl_##S##_unpack_single;                                \
        static constexpr auto for_pack = fl_##S##_for_pack;                                          \
        static constexpr auto unfor_pack = fl_##S##_unfor_pack;                                      \
        static constexpr auto delta = fl_##S##_delta;                                                \
        static constexpr auto undelta = fl_##S##_undelta;                                            \
        static constexpr auto undelta_pack = fl_##S##_undelta_pack;                                  \
        static constexpr auto transpose = fl_##S##_transpose;                                        \
        static constexpr auto untranspose = fl_##S##_untranspose;                                    \
        static constexpr auto undelta_pack_untranspose = fl_##S##_undelta_pack_untranspose;          \
        static constexpr auto transpose_delta_pack = fl_##S##_transpose_delta_pack;                  \
        static constexpr auto unpack_block_sums = fl_##S##_unpack_block_sums;                        \
        static constexpr auto block_min_max = fl_##S##_block_min_max;                                \
        static constexpr auto unpack_compare = fl_##S##_unpack_compare;                              \
        static constexpr auto unfor_compare = fl_##S##_unfor_compare;                                \
        static constexpr auto unfor_compare_widths = fl_##S##_unfor_compare_widths;                  \
        static constexpr auto unfor_compare_range = fl_##S##_unfor_compare_range;                    \
        static constexpr auto unfor_compare_range_widths = fl_##S##_unfor_compare_range_widths;      \
        static constexpr auto unfor_compare_in = fl_##S##_unfor_compare_in;                          \
        static constexpr auto unfor_compare_in_widths = fl_##S##_unfor_compare_in_widths;            \
        static constexpr auto unfor_set_build = fl_##S##_unfor_set_build;                            \
        static constexpr auto unfor_set_build_widths = fl_##S##_unfor_set_build_widths;              \
        static constexpr auto unfor_aggregate_by_window = fl_##S##_unfor_aggregate_by_window;        \
        static constexpr auto unfor_aggregate_by_window_widths = fl_##S##_unfor_aggregate_by_window_widths; \
        static constexpr auto unfor_lookup = fl_##S##_unfor_lookup;                                  \
        static constexpr auto unfor_lookup_widths = fl_##S##_unfor_lookup_widths;                    \
        static constexpr auto unfor_lookup_u8 = fl_##S##_unfor_lookup_u8;                            \
        static constexpr auto unfor_lookup_u8_widths = fl_##S##_unfor_lookup_u8_widths;              \
        static constexpr auto unfor_aggregate_by_lookup = fl_##S##_unfor_aggregate_by_lookup;        \
        static constexpr auto unfor_aggregate_by_lookup_widths = fl_##S##_unfor_aggregate_by_lookup_widths; \
        static constexpr auto undelta_compare_range = fl_##S##_undelta_compare_range;                \
        static constexpr auto undelta_compare_range_widths = fl_##S##_undelta_compare_range_widths;  \
        static constexpr auto undelta_aggregate = fl_##S##_undelta_aggregate;                        \
        static constexpr auto undelta_aggregate_widths = fl_##S##_undelta_aggregate_widths;          \
        static constexpr auto undelta_select = fl_##S##_undelta_select;                              \
        static constexpr auto undelta_select_widths = fl_##S##_undelta_select_widths;                \
        static constexpr auto unfor_compare_columns = fl_##S##_unfor_compare_columns;                \
        static constexpr auto unfor_compare_columns_widths = fl_##S##_unfor_compare_columns_widths;  \
        static constexpr auto unfor_select = fl_##S##_unfor_select;                                  \
        static constexpr auto unfor_select_widths = fl_##S##_unfor_select_widths;                    \
        static constexpr auto unfor_aggregate = fl_##S##_unfor_aggregate;                            \
        static constexpr auto unfor_aggregate_widths = fl_##S##_unfor_aggregate_widths;              \
        static constexpr auto unfor_aggregate_by = fl_##S##_unfor_aggregate_by;                      \
        static constexpr auto unfor_aggregate_by_widths = fl_##S##_unfor_aggregate_by_widths;        \
        static constexpr auto unfor_aggregate_columns = fl_##S##_unfor_aggregate_columns;            \
        static constexpr auto unfor_aggregate_columns_widths = fl_##S##_unfor_aggregate_columns_widths; \
        static constexpr auto unfor_aggregate_by_columns = fl_##S##_unfor_aggregate_by_columns;      \
        static constexpr auto unfor_aggregate_by_columns_widths = fl_##S##_unfor_aggregate_by_columns_widths; \
        static constexpr auto unpack_mixed = fl_##S##_unpack_mixed;                                  \
        static constexpr auto pack_mixed = fl_##S##_pack_mixed;                                      \
        static constexpr auto unpack_widths = fl_##S##_unpack_widths;                                \
        static constexpr auto pack_widths = fl_##S##_pack_widths;                                    \
        static constexpr auto unpack_single_widths = fl_##S##_unpack_single_widths;                  \
        static constexpr auto unfor_pack_widths = fl_##S##_unfor_pack_widths;                        \
        static constexpr auto for_pack_widths = fl_##S##_for_pack_widths;                            \
        static constexpr auto undelta_pack_widths = fl_##S##_undelta_pack_widths;                    \
        static constexpr auto undelta_pack_untranspose_widths = fl_##S##_undelta_pack_untranspose_widths; \
        static constexpr auto transpose_delta_pack_widths = fl_##S##_transpose_delta_pack_widths;    \
        static constexpr auto for_widths = fl_##S##_for_widths;                                      \
        static constexpr auto unpack_batch = fl_##S##_unpack_batch;                                  \
        static constexpr auto pack_batch = fl_##S##_pack_batch;                                      \
        static constexpr auto unfor_pack_batch = fl_##S##_unfor_pack_batch;                          \
        static constexpr auto for_pack_batch = fl_##S##_for_pack_batch;                              \
        static constexpr auto undelta_pack_batch = fl_##S##_undelta_pack_batch;                      \
        static constexpr auto transpose_delta_pack_batch = fl_##S##_transpose_delta_pack_batch;      \
        static constexpr auto pack_host = fl_##S##_pack_host;                                        \
        static constexpr auto unpack_host = fl_##S##_unpack_host;                                    \
        static constexpr auto unpack_single_host = fl_##S##_unpack_single_host;                      \
        static constexpr auto for_pack_host = fl_##S##_for_pack_host;                                \
        static constexpr auto unfor_pack_host = fl_##S##_unfor_pack_host;                            \
        static constexpr auto delta_host = fl_##S##_delta_host;                                      \
        static constexpr auto undelta_host = fl_##S##_undelta_host;                                  \
        static constexpr auto undelta_pack_host = fl_##S##_undelta_pack_host;                        \
        static constexpr auto transpose_host = fl_##S##_transpose_host;                              \
        static constexpr auto untranspose_host = fl_##S##_untranspose_host;                          \
    };
FASTLANES_ABI(std::uint8_t, u8)
FASTLANES_ABI(std::uint16_t, u16)
FASTLANES_ABI(std::uint32_t, u32)
FASTLANES_ABI(std::uint64_t, u64)
#undef FASTLANES_ABI
}  // namespace detail

// lib.rs:24-32
template <typename T> struct FastLanes {
    static constexpr std::size_t T_BITS = sizeof(T) * 8;   // `const T`
    static constexpr std::size_t LANES = 1024 / T_BITS;
};

// bitpacking.rs:16-59
template <typename T> struct BitPacking : FastLanes<T> {
    using A = detail::Abi<T>;
    static constexpr std::size_t TB = sizeof(T) * 8;

    template <std::size_t W> static void pack(const T (&input)[1024], T (&output)[W ? 1024 * W / TB : 1])
    {
        static_assert(W <= TB, "BitPackWidth<W>: SupportedBitPackWidth<T> (bitpacking.rs:8-13)");
        detail::check(A::pack_host(W, input, output, 1), "pack");
    }
    template <std::size_t W> static void unpack(const T (&input)[W ? 1024 * W / TB : 1], T (&output)[1024])
    {
        static_assert(W <= TB, "BitPackWidth<W>: SupportedBitPackWidth<T>");
        detail::check(A::unpack_host(W, input, output, 1), "unpack");
    }
    template <std::size_t W> static T unpack_single(const T (&packed)[W ? 1024 * W / TB : 1], std::size_t index)
    {
        static_assert(W <= TB, "BitPackWidth<W>: SupportedBitPackWidth<T>");
        T v{};
        detail::check(A::unpack_single_host(W, packed, 1, index, &v), "unpack_single");
        return v;
    }
    // bitpacking.rs:76-96 -- lengths as in the debug_asserts (:78-80)
    static void unchecked_pack(std::size_t width, const T* input, std::size_t in_len, T* output, std::size_t out_len)
    {
        if (width > TB) throw Error(FL_ERR_WIDTH, "unchecked_pack");
        if (in_len != 1024 || out_len != 128 * width / sizeof(T)) throw std::length_error("unchecked_pack: buffer sizes");
        detail::check(A::pack_host((unsigned)width, input, output, 1), "unchecked_pack");
    }
    // bitpacking.rs:109-129
    static void unchecked_unpack(std::size_t width, const T* input, std::size_t in_len, T* output, std::size_t out_len)
    {
        if (width > TB) throw Error(FL_ERR_WIDTH, "unchecked_unpack");
        if (out_len != 1024 || in_len != 128 * width / sizeof(T)) throw std::length_error("unchecked_unpack: buffer sizes");
        detail::check(A::unpack_host((unsigned)width, input, output, 1), "unchecked_unpack");
    }
    // bitpacking.rs:181-200
    static T unchecked_unpack_single(std::size_t width, const T* packed, std::size_t len, std::size_t index)
    {
        if (width > TB) throw Error(FL_ERR_WIDTH, "unchecked_unpack_single");
        if (len != 128 * width / sizeof(T)) throw std::length_error("unchecked_unpack_single: buffer size");
        T v{};
        detail::check(A::unpack_single_host((unsigned)width, packed, 1, index, &v), "unchecked_unpack_single");
        return v;
    }
    // batched, device-resident forms (stream = hipStream_t)
    static void pack_device(std::size_t width, const T* d_in, T* d_out, std::size_t n_blocks, void* stream = nullptr)
    { detail::check(A::pack((unsigned)width, d_in, d_out, n_blocks, stream), "pack_device"); }
    static void unpack_device(std::size_t width, const T* d_in, T* d_out, std::size_t n_blocks, void* stream = nullptr)
    { detail::check(A::unpack((unsigned)width, d_in, d_out, n_blocks, stream), "unpack_device"); }
    // extensions: reductions over what unpack / the unpacked block hold
    static void unpack_block_sums_device(std::size_t width, const T* d_packed, std::size_t n_blocks, std::uint64_t* d_sums,
                                         void* stream = nullptr)
    { detail::check(A::unpack_block_sums((unsigned)width, d_packed, n_blocks, d_sums, stream), "unpack_block_sums_device"); }
    // mask bit i of block b = (unpack(block b)[i] <op> constant); 32 words per block
    static void unpack_compare_device(std::size_t width, const T* d_packed, fl_cmp op, T constant, std::size_t n_blocks,
                                      std::uint32_t* d_mask, void* stream = nullptr)
    { detail::check(A::unpack_compare((unsigned)width, d_packed, (int)op, constant, n_blocks, d_mask, stream), "unpack_compare_device"); }
    static void block_min_max_device(const T* d_values, std::size_t n_blocks, T* d_mins, T* d_maxs, void* stream = nullptr)
    { detail::check(A::block_min_max(d_values, n_blocks, d_mins, d_maxs, stream), "block_min_max_device"); }
    static void unpack_single_device(std::size_t width, const T* d_packed, std::size_t n_blocks, const std::uint64_t* d_indices,
                                     std::size_t n_indices, T* d_out, std::uint32_t* d_err, void* stream = nullptr)
    { detail::check(A::unpack_single((unsigned)width, d_packed, n_blocks, d_indices, n_indices, d_out, d_err, stream), "unpack_single_device"); }
};

// ffor.rs:4-18
template <typename T> struct FoR : BitPacking<T> {
    using A = detail::Abi<T>;
    static constexpr std::size_t TB = sizeof(T) * 8;
    template <std::size_t W> static void for_pack(const T (&input)[1024], T reference, T (&output)[W ? 1024 * W / TB : 1])
    {
        static_assert(W <= TB, "BitPackWidth<W>: SupportedBitPackWidth<T>");
        detail::check(A::for_pack_host(W, input, reference, output, 1), "for_pack");
    }
    template <std::size_t W> static void unfor_pack(const T (&input)[W ? 1024 * W / TB : 1], T reference, T (&output)[1024])
    {
        static_assert(W <= TB, "BitPackWidth<W>: SupportedBitPackWidth<T>");
        detail::check(A::unfor_pack_host(W, input, reference, output, 1), "unfor_pack");
    }
    static void for_pack_device(std::size_t width, const T* d_in, const T* d_refs, std::size_t ref_stride, T* d_out,
                                std::size_t n_blocks, void* stream = nullptr)
    { detail::check(A::for_pack((unsigned)width, d_in, d_refs, ref_stride, d_out, n_blocks, stream), "for_pack_device"); }
    static void unfor_pack_device(std::size_t width, const T* d_in, const T* d_refs, std::size_t ref_stride, T* d_out,
                                  std::size_t n_blocks, void* stream = nullptr)
    { detail::check(A::unfor_pack((unsigned)width, d_in, d_refs, ref_stride, d_out, n_blocks, stream), "unfor_pack_device"); }
    // mask bit i of block b = (unfor_pack(block b, d_refs[b * ref_stride])[i] <op> constant); 32 words per block
    static void unfor_compare_device(std::size_t width, const T* d_packed, const T* d_refs, std::size_t ref_stride, fl_cmp op, T constant,
                                     std::size_t n_blocks, std::uint32_t* d_mask, void* stream = nullptr)
    { detail::check(A::unfor_compare((unsigned)width, d_packed, d_refs, ref_stride, (int)op, constant, n_blocks, d_mask, stream), "unfor_compare_device"); }
    // the cyclic interval [lo, hi] (mod 2^T) over the same values, joined with the mask so far: FL_MASK_NEW (d_mask_in unused, may be
    // nullptr), FL_MASK_AND, FL_MASK_OR; d_mask may be d_mask_in itself
    static void unfor_compare_range_device(std::size_t width, const T* d_packed, const T* d_refs, std::size_t ref_stride, T lo, T hi,
                                           fl_mask_combine combine, const std::uint32_t* d_mask_in, std::size_t n_blocks, std::uint32_t* d_mask,
                                           void* stream = nullptr)
    { detail::check(A::unfor_compare_range((unsigned)width, d_packed, d_refs, ref_stride, lo, hi, (int)combine, d_mask_in, n_blocks, d_mask, stream), "unfor_compare_range_device"); }
    // set membership over the same values: v is a member when j = (v - set_lo) mod 2^T < set_bits and bit j of d_set_words is set
    // (negate: NOT IN), joined with the mask so far as unfor_compare_range_device does; set_bits == 0 is the empty set
    static void unfor_compare_in_device(std::size_t width, const T* d_packed, const T* d_refs, std::size_t ref_stride, T set_lo,
                                        std::uint64_t set_bits, const std::uint32_t* d_set_words, bool negate, fl_mask_combine combine,
                                        const std::uint32_t* d_mask_in, std::size_t n_blocks, std::uint32_t* d_mask, void* stream = nullptr)
    { detail::check(A::unfor_compare_in((unsigned)width, d_packed, d_refs, ref_stride, set_lo, set_bits, d_set_words, negate ? 1 : 0, (int)combine, d_mask_in, n_blocks, d_mask, stream), "unfor_compare_in_device"); }
    // the member set unfor_compare_in_device probes, built from the same values: every value v of a row d_mask keeps (nullptr: every
    // row) sets bit j = (v - set_lo) mod 2^T of d_set_words when j < set_bits; d_stats (nullptr: not counted) += {kept rows inside the
    // window, kept rows outside}.  ORs and adds, never clears: zero d_set_words and d_stats first, or pass an earlier call's
    static void unfor_set_build_device(std::size_t width, const T* d_packed, const T* d_refs, std::size_t ref_stride, const std::uint32_t* d_mask,
                                       std::size_t n_blocks, T set_lo, std::uint64_t set_bits, std::uint32_t* d_set_words,
                                       std::uint64_t* d_stats = nullptr, void* stream = nullptr)
    { detail::check(A::unfor_set_build((unsigned)width, d_packed, d_refs, ref_stride, d_mask, n_blocks, set_lo, set_bits, d_set_words, d_stats, stream), "unfor_set_build_device"); }
    // GROUP BY a key column of the same type inside the window [key_lo, key_lo + n_groups - 1]: every row d_mask keeps (nullptr: every
    // row) whose key k has j = (k - key_lo) mod 2^T < n_groups updates d_counts[j] / d_sums[j] / d_mins[j] / d_maxs[j] (uint64[n_groups]
    // each; nullptr: not maintained) with its value; d_stats (nullptr: not counted) += {kept rows inside the window, kept rows outside}.
    // Accumulates, never clears: write the identities 0 / 0 / UINT64_MAX / 0 first, or pass an earlier call's arrays
    static void unfor_aggregate_by_window_device(std::size_t width, const T* d_packed, const T* d_refs, std::size_t ref_stride, std::size_t key_width,
                                                 const T* d_keys, const T* d_key_refs, std::size_t key_ref_stride, const std::uint32_t* d_mask,
                                                 std::size_t n_blocks, T key_lo, std::uint64_t n_groups, std::uint64_t* d_counts, std::uint64_t* d_sums,
                                                 std::uint64_t* d_mins, std::uint64_t* d_maxs, std::uint64_t* d_stats = nullptr, void* stream = nullptr)
    { detail::check(A::unfor_aggregate_by_window((unsigned)width, d_packed, d_refs, ref_stride, (unsigned)key_width, d_keys, d_key_refs, key_ref_stride, d_mask, n_blocks, key_lo, n_groups, d_counts, d_sums, d_mins, d_maxs, d_stats, stream), "unfor_aggregate_by_window_device"); }
    // the probe side of a payload join: d_out block b = pack::<T bits>(v), v[i] = d_table[j] for a row d_mask keeps (nullptr: every row)
    // whose key k has j = (k - key_lo) mod 2^T < n_slots and bit j of d_present set (nullptr: every slot), `missing` otherwise; d_hit_mask
    // (nullptr: not written; may be d_mask) = the hits, d_stats (nullptr: not counted) += {hits, kept rows that miss}.  d_out is a
    // width-T column with a zero reference: any unfor_* entry point takes it, a second lookup among them
    static void unfor_lookup_device(std::size_t width, const T* d_packed, const T* d_refs, std::size_t ref_stride, const std::uint32_t* d_mask,
                                    std::size_t n_blocks, T key_lo, std::uint64_t n_slots, const T* d_table, const std::uint32_t* d_present, T missing,
                                    T* d_out, std::uint32_t* d_hit_mask = nullptr, std::uint64_t* d_stats = nullptr, void* stream = nullptr)
    { detail::check(A::unfor_lookup((unsigned)width, d_packed, d_refs, ref_stride, d_mask, n_blocks, key_lo, n_slots, d_table, d_present, missing, d_out, d_hit_mask, d_stats, stream), "unfor_lookup_device"); }
    // ... with a uint8_t payload (for T = u8 the function above): d_out holds the 1024 values of a block in row order -- as it stands the u8 key
    // column (key_width 8, one zero reference, stride 0) of unfor_aggregate_by_device and unfor_aggregate_by_columns_device
    static void unfor_lookup_u8_device(std::size_t width, const T* d_packed, const T* d_refs, std::size_t ref_stride, const std::uint32_t* d_mask,
                                       std::size_t n_blocks, T key_lo, std::uint64_t n_slots, const std::uint8_t* d_table,
                                       const std::uint32_t* d_present, std::uint8_t missing, std::uint8_t* d_out, std::uint32_t* d_hit_mask = nullptr,
                                       std::uint64_t* d_stats = nullptr, void* stream = nullptr)
    { detail::check(A::unfor_lookup_u8((unsigned)width, d_packed, d_refs, ref_stride, d_mask, n_blocks, key_lo, n_slots, d_table, d_present, missing, d_out, d_hit_mask, d_stats, stream), "unfor_lookup_u8_device"); }
    // unfor_lookup_u8_device and unfor_aggregate_by_device in one pass, with no code column and no hit mask written: d_result[g], g = 0 ..
    // 255 (all written by every call), = count / sum / min / max of the values of the rows d_mask keeps (nullptr: every row) whose key k of
    // the key column (the value column's own type) has j = (k - key_lo) mod 2^T < n_slots, bit j of d_present set (nullptr: every slot)
    // and d_table[j] == g; d_stats (nullptr: not counted) += {hits, kept rows that miss}
    static void unfor_aggregate_by_lookup_device(std::size_t width, const T* d_packed, const T* d_refs, std::size_t ref_stride, std::size_t key_width,
                                                 const T* d_keys, const T* d_key_refs, std::size_t key_ref_stride, const std::uint32_t* d_mask,
                                                 std::size_t n_blocks, T key_lo, std::uint64_t n_slots, const std::uint8_t* d_table,
                                                 const std::uint32_t* d_present, fl_block_aggregate* d_result, std::uint64_t* d_stats = nullptr,
                                                 std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
    { detail::check(A::unfor_aggregate_by_lookup((unsigned)width, d_packed, d_refs, ref_stride, (unsigned)key_width, d_keys, d_key_refs, key_ref_stride, d_mask, n_blocks, key_lo, n_slots, d_table, d_present, d_result, d_stats, d_err_flag, stream), "unfor_aggregate_by_lookup_device"); }
    // a <op> b between two FoR-packed columns of T with the same block count (signed: of the two's-complement values), joined with the
    // mask so far as unfor_compare_range_device does; a block pair the references and widths decide reads neither column
    static void unfor_compare_columns_device(std::size_t width_a, const T* d_a, const T* d_a_refs, std::size_t a_ref_stride, std::size_t width_b,
                                             const T* d_b, const T* d_b_refs, std::size_t b_ref_stride, fl_cmp op, bool is_signed,
                                             fl_mask_combine combine, const std::uint32_t* d_mask_in, std::size_t n_blocks, std::uint32_t* d_mask,
                                             void* stream = nullptr)
    { detail::check(A::unfor_compare_columns((unsigned)width_a, d_a, d_a_refs, a_ref_stride, (unsigned)width_b, d_b, d_b_refs, b_ref_stride, (int)op, is_signed ? 1 : 0, (int)combine, d_mask_in, n_blocks, d_mask, stream), "unfor_compare_columns_device"); }
    // only the values of unfor_pack(..) whose mask bit is set, compacted: block b's go to d_out[d_out_offsets[b] ..] (mask_offsets_device)
    static void unfor_select_device(std::size_t width, const T* d_packed, const T* d_refs, std::size_t ref_stride, const std::uint32_t* d_mask,
                                    const std::uint64_t* d_out_offsets, T* d_out, std::size_t out_len, std::size_t n_blocks,
                                    std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
    { detail::check(A::unfor_select((unsigned)width, d_packed, d_refs, ref_stride, d_mask, d_out_offsets, d_out, out_len, n_blocks, d_err_flag, stream), "unfor_select_device"); }
    // count / sum / min / max per block of the values of unfor_pack(..) whose mask bit is set (d_mask == nullptr: of all of them), never
    // materialised: d_block_aggs[b] for every block; aggregate_reduce_device combines them
    static void unfor_aggregate_device(std::size_t width, const T* d_packed, const T* d_refs, std::size_t ref_stride, const std::uint32_t* d_mask,
                                       std::size_t n_blocks, fl_block_aggregate* d_block_aggs, std::uint32_t* d_err_flag = nullptr,
                                       void* stream = nullptr)
    { detail::check(A::unfor_aggregate((unsigned)width, d_packed, d_refs, ref_stride, d_mask, n_blocks, d_block_aggs, d_err_flag, stream), "unfor_aggregate_device"); }
    // the same grouped by a FoR-packed u8 key column of the same block count: d_result[g], g = 0 .. 255, = count / sum / min / max of the
    // kept rows whose key is g (the identity where there are none); all 256 slots are written by every call
    static void unfor_aggregate_by_device(std::size_t width, const T* d_packed, const T* d_refs, std::size_t ref_stride, std::size_t key_width,
                                          const std::uint8_t* d_keys, const std::uint8_t* d_key_refs, std::size_t key_ref_stride,
                                          const std::uint32_t* d_mask, std::size_t n_blocks, fl_block_aggregate* d_result,
                                          std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
    { detail::check(A::unfor_aggregate_by((unsigned)width, d_packed, d_refs, ref_stride, (unsigned)key_width, d_keys, d_key_refs, key_ref_stride, d_mask, n_blocks, d_result, d_err_flag, stream), "unfor_aggregate_by_device"); }
    // count / sum / min / max per block of a * b, a + b or a - b between two FoR-packed columns of T with the same block count, the values
    // zero-extended to 64 bits first (a negative difference is its two's-complement pattern; min / max compare the patterns unsigned), over
    // the rows whose mask bit is set (d_mask == nullptr: every row); neither column is materialised; aggregate_reduce_device combines the slots
    static void unfor_aggregate_columns_device(fl_expr expr, std::size_t width_a, const T* d_a, const T* d_a_refs, std::size_t a_ref_stride,
                                               std::size_t width_b, const T* d_b, const T* d_b_refs, std::size_t b_ref_stride,
                                               const std::uint32_t* d_mask, std::size_t n_blocks, fl_block_aggregate* d_block_aggs,
                                               std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
    { detail::check(A::unfor_aggregate_columns((int)expr, (unsigned)width_a, d_a, d_a_refs, a_ref_stride, (unsigned)width_b, d_b, d_b_refs, b_ref_stride, d_mask, n_blocks, d_block_aggs, d_err_flag, stream), "unfor_aggregate_columns_device"); }
    // the same expression grouped by a FoR-packed u8 key column of the same block count: d_result[g] (256 slots, all written by every call)
    // = count / sum / min / max of a * b, a + b or a - b over the kept rows whose key is g; none of the three columns is materialised
    static void unfor_aggregate_by_columns_device(fl_expr expr, std::size_t width_a, const T* d_a, const T* d_a_refs, std::size_t a_ref_stride,
                                                  std::size_t width_b, const T* d_b, const T* d_b_refs, std::size_t b_ref_stride,
                                                  std::size_t key_width, const std::uint8_t* d_keys, const std::uint8_t* d_key_refs,
                                                  std::size_t key_ref_stride, const std::uint32_t* d_mask, std::size_t n_blocks,
                                                  fl_block_aggregate* d_result, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
    { detail::check(A::unfor_aggregate_by_columns((int)expr, (unsigned)width_a, d_a, d_a_refs, a_ref_stride, (unsigned)width_b, d_b, d_b_refs, b_ref_stride, (unsigned)key_width, d_keys, d_key_refs, key_ref_stride, d_mask, n_blocks, d_result, d_err_flag, stream), "unfor_aggregate_by_columns_device"); }
};

// delta.rs:6-17
template <typename T> struct Delta : BitPacking<T> {
    using A = detail::Abi<T>;
    static constexpr std::size_t TB = sizeof(T) * 8;
    static constexpr std::size_t LANES = 1024 / TB;
    static void delta(const T (&input)[1024], const T (&base)[LANES], T (&output)[1024])
    { detail::check(A::delta_host(input, base, output, 1), "delta"); }
    static void undelta(const T (&input)[1024], const T (&base)[LANES], T (&output)[1024])
    { detail::check(A::undelta_host(input, base, output, 1), "undelta"); }
    template <std::size_t W>
    static void undelta_pack(const T (&input)[W ? 1024 * W / TB : 1], const T (&base)[LANES], T (&output)[1024])
    {
        static_assert(W <= TB, "BitPackWidth<W>: SupportedBitPackWidth<T>");
        detail::check(A::undelta_pack_host(W, input, base, output, 1), "undelta_pack");
    }
    static void delta_device(const T* d_in, const T* d_bases, T* d_out, std::size_t n_blocks, void* stream = nullptr)
    { detail::check(A::delta(d_in, d_bases, d_out, n_blocks, stream), "delta_device"); }
    static void undelta_device(const T* d_in, const T* d_bases, T* d_out, std::size_t n_blocks, void* stream = nullptr)
    { detail::check(A::undelta(d_in, d_bases, d_out, n_blocks, stream), "undelta_device"); }
    static void undelta_pack_device(std::size_t width, const T* d_in, const T* d_bases, T* d_out, std::size_t n_blocks,
                                    void* stream = nullptr)
    { detail::check(A::undelta_pack((unsigned)width, d_in, d_bases, d_out, n_blocks, stream), "undelta_pack_device"); }
    // extensions: == untranspose(undelta_pack(..)) / pack(delta(transpose(..)))  (delta.rs:88-100)
    static void undelta_pack_untranspose_device(std::size_t width, const T* d_in, const T* d_bases, T* d_out,
                                                std::size_t n_blocks, void* stream = nullptr)
    { detail::check(A::undelta_pack_untranspose((unsigned)width, d_in, d_bases, d_out, n_blocks, stream), "undelta_pack_untranspose_device"); }
    // the cyclic interval [lo, hi] (mod 2^T) over the values undelta_pack_untranspose_device yields (ORIGINAL row order), joined with
    // the mask so far exactly as FoR<T>::unfor_compare_range_device joins it (the same masks; d_mask may be d_mask_in): no decoded
    // column is written, a block its bases and width decide reads no packed byte
    static void undelta_compare_range_device(std::size_t width, const T* d_packed, const T* d_bases, T lo, T hi, fl_mask_combine combine,
                                             const std::uint32_t* d_mask_in, std::size_t n_blocks, std::uint32_t* d_mask, void* stream = nullptr)
    { detail::check(A::undelta_compare_range((unsigned)width, d_packed, d_bases, lo, hi, (int)combine, d_mask_in, n_blocks, d_mask, stream), "undelta_compare_range_device"); }
    // COUNT / SUM / MIN / MAX per block of the rows d_mask keeps (nullptr: every row) of the Delta-packed column, in original row order:
    // d_block_aggs[b] as FoR<T>::unfor_aggregate_device writes it, reduced by aggregate_reduce_device; no decoded column is written
    static void undelta_aggregate_device(std::size_t width, const T* d_packed, const T* d_bases, const std::uint32_t* d_mask, std::size_t n_blocks,
                                         fl_block_aggregate* d_block_aggs, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
    { detail::check(A::undelta_aggregate((unsigned)width, d_packed, d_bases, d_mask, n_blocks, d_block_aggs, d_err_flag, stream), "undelta_aggregate_device"); }
    // the rows d_mask keeps of the Delta-packed column, compacted in original row order: block b's run at d_out + d_out_offsets[b]
    // (mask_offsets_device's results), as FoR<T>::unfor_select_device writes it; no full-width decoded column is written
    static void undelta_select_device(std::size_t width, const T* d_packed, const T* d_bases, const std::uint32_t* d_mask,
                                      const std::uint64_t* d_out_offsets, T* d_out, std::size_t out_len, std::size_t n_blocks,
                                      std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
    { detail::check(A::undelta_select((unsigned)width, d_packed, d_bases, d_mask, d_out_offsets, d_out, out_len, n_blocks, d_err_flag, stream), "undelta_select_device"); }
    static void transpose_delta_pack_device(std::size_t width, const T* d_in, const T* d_bases, T* d_out,
                                            std::size_t n_blocks, void* stream = nullptr)
    { detail::check(A::transpose_delta_pack((unsigned)width, d_in, d_bases, d_out, n_blocks, stream), "transpose_delta_pack_device"); }
};

// transpose.rs:4-7,29-36
constexpr std::size_t transpose(std::size_t idx)
{
    return (idx % 16) * 64 + FL_ORDER[(idx / 16) % 8] * 8 + idx / 128;
}
template <typename T> struct Transpose : FastLanes<T> {
    using A = detail::Abi<T>;
    static void transpose(const T (&input)[1024], T (&output)[1024])
    { detail::check(A::transpose_host(input, output, 1), "transpose"); }
    static void untranspose(const T (&input)[1024], T (&output)[1024])
    { detail::check(A::untranspose_host(input, output, 1), "untranspose"); }
    static void transpose_device(const T* d_in, T* d_out, std::size_t n_blocks, void* stream = nullptr)
    { detail::check(A::transpose(d_in, d_out, n_blocks, stream), "transpose_device"); }
    static void untranspose_device(const T* d_in, T* d_out, std::size_t n_blocks, void* stream = nullptr)
    { detail::check(A::untranspose(d_in, d_out, n_blocks, stream), "untranspose_device"); }
};

// ---------------------------------------------------------------------------------------------------------------------
// The reference's CALLER LOOP as one checked call.  Vortex (and benches/bitpacking.rs:80-97) hold a column as slices and loop
//     for i in 0..n { T::unchecked_unpack(w, &packed[i*pl..(i+1)*pl], &mut out[i*1024..(i+1)*1024]) }
// where every iteration asserts its two lengths (bitpacking.rs:78-80, :111-113).  A DeviceSlice is the device-resident
// counterpart of such a slice -- pointer AND element count -- and the *_column functions below check the same lengths for the
// whole column before the one asynchronous launch, so the fast path keeps what the slow path asserted.  A length mismatch
// throws std::length_error (the reference's debug_assert), width > T throws Error(FL_ERR_WIDTH) (its unreachable!()).
// (bindings/rust/src/device.rs is the same surface in Rust.)
// ---------------------------------------------------------------------------------------------------------------------
template <typename T> struct DeviceSlice {
    T* ptr = nullptr;          // device pointer, 16-byte aligned
    std::size_t len = 0;       // elements
    DeviceSlice() = default;
    DeviceSlice(T* p, std::size_t n) : ptr(p), len(n) {}
    template <typename U, typename = std::enable_if_t<std::is_same<const U, T>::value>>
    DeviceSlice(const DeviceSlice<U>& o) : ptr(o.ptr), len(o.len) {}          // DeviceSlice<T> -> DeviceSlice<const T>
    // elements [first, first + count): the sub-slice a sharded caller hands each device / stream
    DeviceSlice subslice(std::size_t first, std::size_t count) const
    {
        if (first > len || count > len - first) throw std::out_of_range("DeviceSlice::subslice");
        return DeviceSlice(ptr + first, count);
    }
};

namespace detail {
// number of 1024-value blocks of a column given as (packed, unpacked) slices of width `width`; throws unless
// unpacked.len == 1024 * n and packed.len == n * 1024 * width / T for one n  (bitpacking.rs:78-80, :111-113 for every block)
template <typename T>
inline std::size_t column_blocks(std::size_t width, std::size_t packed_len, std::size_t unpacked_len, const char* where)
{
    constexpr std::size_t TB = sizeof(T) * 8;
    if (width > TB) throw Error(FL_ERR_WIDTH, where);
    if (unpacked_len % 1024 != 0) throw std::length_error(std::string(where) + ": the unpacked slice must hold 1024 elements per block");
    const std::size_t n = unpacked_len / 1024;
    if (packed_len != n * (1024 * width / TB))
        throw std::length_error(std::string(where) + ": the packed slice must hold 1024 * W / T elements per block");
    return n;
}
}  // namespace detail

// for b in blocks { T::unchecked_unpack(width, &packed[b*pl..], &mut out[b*1024..]) }   (bitpacking.rs:109-129)
template <typename T>
inline void unpack_column(std::size_t width, DeviceSlice<const T> packed, DeviceSlice<T> out, void* stream = nullptr)
{
    const std::size_t n = detail::column_blocks<T>(width, packed.len, out.len, "unpack_column");
    detail::check(detail::Abi<T>::unpack((unsigned)width, packed.ptr, out.ptr, n, stream), "unpack_column");
}
// for b in blocks { T::unchecked_pack(width, &input[b*1024..], &mut packed[b*pl..]) }   (bitpacking.rs:76-96)
template <typename T>
inline void pack_column(std::size_t width, DeviceSlice<const T> input, DeviceSlice<T> packed, void* stream = nullptr)
{
    const std::size_t n = detail::column_blocks<T>(width, packed.len, input.len, "pack_column");
    detail::check(detail::Abi<T>::pack((unsigned)width, input.ptr, packed.ptr, n, stream), "pack_column");
}
// for b in blocks { T::undelta_pack::<W>(&packed[b], &bases[b], &mut out[b]) }   (delta.rs:47-63); bases: LANES per block
template <typename T>
inline void undelta_pack_column(std::size_t width, DeviceSlice<const T> packed, DeviceSlice<const T> bases, DeviceSlice<T> out,
                                void* stream = nullptr)
{
    const std::size_t n = detail::column_blocks<T>(width, packed.len, out.len, "undelta_pack_column");
    if (bases.len != n * (1024 / (sizeof(T) * 8))) throw std::length_error("undelta_pack_column: bases must hold LANES elements per block");
    detail::check(detail::Abi<T>::undelta_pack((unsigned)width, packed.ptr, bases.ptr, out.ptr, n, stream), "undelta_pack_column");
}
// for b in blocks { T::unfor_pack::<W>(&packed[b], references[b], &mut out[b]) }   (ffor.rs:38-50); one reference per block,
// or ONE for the whole column (references.len == 1)
template <typename T>
inline void unfor_pack_column(std::size_t width, DeviceSlice<const T> packed, DeviceSlice<const T> references, DeviceSlice<T> out,
                              void* stream = nullptr)
{
    const std::size_t n = detail::column_blocks<T>(width, packed.len, out.len, "unfor_pack_column");
    if (references.len != n && references.len != 1) throw std::length_error("unfor_pack_column: one reference per block, or one in all");
    detail::check(detail::Abi<T>::unfor_pack((unsigned)width, packed.ptr, references.ptr, references.len == 1 ? 0 : 1, out.ptr, n, stream),
                  "unfor_pack_column");
}

// The same loop over MANY SMALL ARRAYS ("chunks": Vortex keeps 64 Ki values per chunk), one launch: the four per-chunk device
// arrays of fl_<ty>_unpack_batch with their lengths.  unpack_chunks checks that the table is consistent (one entry per chunk in
// every array); what only the device can see -- each chunk's width, pointers' alignment, block count against max_blocks -- is
// checked by the kernel and reported through *err_flag (FL_DEVERR_*).
template <typename T> struct ChunkTable {
    DeviceSlice<const T* const> packed;          // [n_chunks] device pointers to the chunks' packed blocks
    DeviceSlice<T* const> out;                   // [n_chunks] device pointers to where each chunk decodes
    DeviceSlice<const std::uint8_t> widths;      // [n_chunks]
    DeviceSlice<const std::uint32_t> n_blocks;   // [n_chunks]
    std::uint32_t max_blocks = 0;                // host-side bound on n_blocks[c] (sizes the grid)
};
template <typename T>
inline void unpack_chunks(const ChunkTable<T>& t, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{
    const std::size_t n = t.widths.len;
    if (t.packed.len != n || t.out.len != n || t.n_blocks.len != n) throw std::length_error("unpack_chunks: every array of the table holds one entry per chunk");
    detail::check(detail::Abi<T>::unpack_batch(t.packed.ptr, t.out.ptr, t.widths.ptr, t.n_blocks.ptr, n, t.max_blocks, d_err_flag, stream), "unpack_chunks");
}
// A column whose blocks each have their own width: the caller loop
// `for b { T::unchecked_unpack(widths[b], ..) }` (bitpacking.rs:109-129) as one device call.
template <typename T> class MixedWidthPlan {
public:
    MixedWidthPlan(const std::uint8_t* widths, std::size_t n_blocks)
    { detail::check(fl_mixed_plan_create(sizeof(T) * 8, widths, n_blocks, &plan_), "fl_mixed_plan_create"); }
    ~MixedWidthPlan() { fl_mixed_plan_destroy(plan_); }
    MixedWidthPlan(const MixedWidthPlan&) = delete;
    MixedWidthPlan& operator=(const MixedWidthPlan&) = delete;
    std::size_t n_blocks() const { return fl_mixed_plan_n_blocks(plan_); }
    std::uint64_t packed_bytes() const { return fl_mixed_plan_packed_bytes(plan_); }
    void unpack_device(const T* d_packed, T* d_out, void* stream = nullptr) const
    { detail::check(detail::Abi<T>::unpack_mixed(plan_, d_packed, d_out, stream), "unpack_mixed"); }
    void pack_device(const T* d_in, T* d_packed, void* stream = nullptr) const
    { detail::check(detail::Abi<T>::pack_mixed(plan_, d_in, d_packed, stream), "pack_mixed"); }
    const std::uint8_t* widths_device() const { return fl_mixed_plan_widths(plan_); }
    const std::uint64_t* offsets_device() const { return fl_mixed_plan_offsets(plan_); }
private:
    fl_mixed_plan* plan_ = nullptr;
};

// The optional allocation helper of fastlanes_amd.h as an owner: a (packed, unpacked) buffer pair for a column of `packed_len` /
// `unpacked_len` ELEMENTS (either direction: in = what the op reads), placed by measurement by default (FL_LAYOUT_PROBE:
// synchronous, contents unspecified afterwards).  Never needed to use the codec -- every call above takes any aligned pointers.
template <typename T> class ColumnPair {
public:
    ColumnPair(std::size_t in_len, std::size_t out_len, std::size_t aux_len = 0, int layout = FL_LAYOUT_PROBE, void* stream = nullptr)
    {
        void *i = nullptr, *a = nullptr, *o = nullptr;
        detail::check(fl_column_pair_alloc(in_len * sizeof(T), aux_len * sizeof(T), out_len * sizeof(T), layout, stream, &i, &a, &o, &handle_,
                                           &layout_, probe_gbps_), "fl_column_pair_alloc");
        in_ = DeviceSlice<T>(static_cast<T*>(i), in_len);
        aux_ = DeviceSlice<T>(static_cast<T*>(a), aux_len);
        out_ = DeviceSlice<T>(static_cast<T*>(o), out_len);
    }
    ~ColumnPair() { fl_column_pair_free(handle_); }
    ColumnPair(const ColumnPair&) = delete;
    ColumnPair& operator=(const ColumnPair&) = delete;
    DeviceSlice<T> in() const { return in_; }
    DeviceSlice<T> aux() const { return aux_; }
    DeviceSlice<T> out() const { return out_; }
    int layout() const { return layout_; }                                  // FL_LAYOUT_SEPARATE / _ZONED / _INTERLEAVED: what was kept
    std::uint32_t probe_gbps(int layout) const { return layout >= 0 && layout < FL_LAYOUT_COUNT ? probe_gbps_[layout] : 0; }   // 0 = not measured
private:
    void* handle_ = nullptr;
    DeviceSlice<T> in_, aux_, out_;
    int layout_ = -1;
    std::uint32_t probe_gbps_[FL_LAYOUT_COUNT] = {0, 0, 0, 0};
};

// The same loop with the per-block widths / byte offsets already resident in HBM:
// nothing is built on the host.  A block with a width > T, a misaligned offset or bytes outside [0, packed_bytes) is skipped and its
// FL_DEVERR_* bit is ORed into *d_err_flag (device uint32, may be null).
template <typename T>
inline void unpack_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes, T* d_out,
                                 std::size_t n_blocks, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unpack_widths(d_widths, d_offsets, d_packed, packed_bytes, d_out, n_blocks, d_err_flag, stream), "unpack_widths"); }
template <typename T>
inline void pack_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_in, T* d_packed, std::size_t packed_bytes,
                               std::size_t n_blocks, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::pack_widths(d_widths, d_offsets, d_in, d_packed, packed_bytes, n_blocks, d_err_flag, stream), "pack_widths"); }
template <typename T>
inline void unpack_single_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                        std::size_t n_blocks, const std::uint64_t* d_indices, std::size_t n_indices, T* d_out,
                                        std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unpack_single_widths(d_widths, d_offsets, d_packed, packed_bytes, n_blocks, d_indices, n_indices, d_out, d_err_flag, stream), "unpack_single_widths"); }
// ... with FoR's / Delta's bodies: `for b { FoR::unfor_pack::<widths[b]>(.., d_references[b * reference_stride], ..) }` (ffor.rs:24-50),
// `for b { Delta::undelta_pack::<widths[b]>(.., &d_bases[b], ..) }` (delta.rs:47-63; `untranspose`: straight to original order), and the
// fused encode `pack::<widths[b]>(delta(transpose(..), &d_bases[b]))`.
template <typename T>
inline void unfor_pack_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                     const T* d_references, std::size_t reference_stride, T* d_out, std::size_t n_blocks,
                                     std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_pack_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, d_out, n_blocks, d_err_flag, stream), "unfor_pack_widths"); }
// the selection mask of the same column: bit i of block b = (unfor_pack::<widths[b]>(..)[i] <op> constant), 32 words per block
template <typename T>
inline void unfor_compare_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                        const T* d_references, std::size_t reference_stride, fl_cmp op, T constant, std::size_t n_blocks,
                                        std::uint32_t* d_mask, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_compare_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, (int)op, constant, n_blocks, d_mask, d_err_flag, stream), "unfor_compare_widths"); }
// ... and an interval predicate chained through the mask so far: mask = [d_mask_in &, |] (value in the cyclic interval [lo, hi]); a block
// the mask so far has already decided (all zero under AND, all ones under OR) is not read; d_mask may be d_mask_in itself
template <typename T>
inline void unfor_compare_range_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                              const T* d_references, std::size_t reference_stride, T lo, T hi, fl_mask_combine combine,
                                              const std::uint32_t* d_mask_in, std::size_t n_blocks, std::uint32_t* d_mask,
                                              std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_compare_range_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, lo, hi, (int)combine, d_mask_in, n_blocks, d_mask, d_err_flag, stream), "unfor_compare_range_widths"); }
// ... and the same interval over a mixed-width DELTA-packed column (d_bases: LANES per block), the values in original row order: the
// head of such a chain on a sorted column; the same device checks, a failing block keeps its mask words
template <typename T>
inline void undelta_compare_range_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                                const T* d_bases, T lo, T hi, fl_mask_combine combine, const std::uint32_t* d_mask_in,
                                                std::size_t n_blocks, std::uint32_t* d_mask, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::undelta_compare_range_widths(d_widths, d_offsets, d_packed, packed_bytes, d_bases, lo, hi, (int)combine, d_mask_in, n_blocks, d_mask, d_err_flag, stream), "undelta_compare_range_widths"); }
// ... and the aggregate such a mask feeds: Delta<T>::undelta_aggregate_device over a mixed-width Delta-packed column (a block that fails
// the device checks leaves the identity in its slot)
template <typename T>
inline void undelta_aggregate_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                            const T* d_bases, const std::uint32_t* d_mask, std::size_t n_blocks, fl_block_aggregate* d_block_aggs,
                                            std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::undelta_aggregate_widths(d_widths, d_offsets, d_packed, packed_bytes, d_bases, d_mask, n_blocks, d_block_aggs, d_err_flag, stream), "undelta_aggregate_widths"); }
// ... and the rows such a mask keeps, materialised: Delta<T>::undelta_select_device over a mixed-width Delta-packed column (a block that
// fails the device checks, or whose run does not fit d_out, is skipped and its output slots are left untouched)
template <typename T>
inline void undelta_select_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                         const T* d_bases, const std::uint32_t* d_mask, const std::uint64_t* d_out_offsets, T* d_out,
                                         std::size_t out_len, std::size_t n_blocks, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::undelta_select_widths(d_widths, d_offsets, d_packed, packed_bytes, d_bases, d_mask, d_out_offsets, d_out, out_len, n_blocks, d_err_flag, stream), "undelta_select_widths"); }
// ... and set membership chained the same way: mask = [d_mask_in &, |] (value in the member set: a window of set_bits values from set_lo,
// one bitmap bit each; negate: NOT IN); a block outside the window, or one the mask so far has decided, is not read
template <typename T>
inline void unfor_compare_in_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                           const T* d_references, std::size_t reference_stride, T set_lo, std::uint64_t set_bits,
                                           const std::uint32_t* d_set_words, bool negate, fl_mask_combine combine, const std::uint32_t* d_mask_in,
                                           std::size_t n_blocks, std::uint32_t* d_mask, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_compare_in_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, set_lo, set_bits, d_set_words, negate ? 1 : 0, (int)combine, d_mask_in, n_blocks, d_mask, d_err_flag, stream), "unfor_compare_in_widths"); }
// ... and the member set such a probe takes, built from a mixed-width column under a mask (the build side of a semi-join): bit
// (v - set_lo) mod 2^T of d_set_words |= 1 for every kept value v inside the window, d_stats += {inside, outside}; never clears
template <typename T>
inline void unfor_set_build_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                          const T* d_references, std::size_t reference_stride, const std::uint32_t* d_mask, std::size_t n_blocks,
                                          T set_lo, std::uint64_t set_bits, std::uint32_t* d_set_words, std::uint64_t* d_stats = nullptr,
                                          std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_set_build_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, d_mask, n_blocks, set_lo, set_bits, d_set_words, d_stats, d_err_flag, stream), "unfor_set_build_widths"); }
// ... and the grouped aggregate of a mixed-width value column by a mixed-width key column of the same type inside a dense window of the
// key domain: d_counts / d_sums / d_mins / d_maxs[(key - key_lo) mod 2^T] are updated for every kept row inside the window (nullptr: not
// maintained), d_stats += {inside, outside}; never clears
template <typename T>
inline void unfor_aggregate_by_window_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                                    const T* d_references, std::size_t reference_stride, const std::uint8_t* d_key_widths,
                                                    const std::uint64_t* d_key_offsets, const T* d_keys, std::size_t keys_bytes, const T* d_key_references,
                                                    std::size_t key_reference_stride, const std::uint32_t* d_mask, std::size_t n_blocks, T key_lo,
                                                    std::uint64_t n_groups, std::uint64_t* d_counts, std::uint64_t* d_sums, std::uint64_t* d_mins,
                                                    std::uint64_t* d_maxs, std::uint64_t* d_stats = nullptr, std::uint32_t* d_err_flag = nullptr,
                                                    void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_aggregate_by_window_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, d_key_widths, d_key_offsets, d_keys, keys_bytes, d_key_references, key_reference_stride, d_mask, n_blocks, key_lo, n_groups, d_counts, d_sums, d_mins, d_maxs, d_stats, d_err_flag, stream), "unfor_aggregate_by_window_widths"); }
// ... and the payload join's probe side over a mixed-width key column: d_out block b = pack::<T bits>(v), v[i] = d_table[(key - key_lo)
// mod 2^T] for a kept row inside the window whose d_present bit is set (nullptr: every slot), `missing` otherwise; d_hit_mask (nullptr: not
// written; may be d_mask) = the hits, d_stats += {hits, kept rows that miss}; a block that fails the device checks is left untouched
template <typename T>
inline void unfor_lookup_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                       const T* d_references, std::size_t reference_stride, const std::uint32_t* d_mask, std::size_t n_blocks, T key_lo,
                                       std::uint64_t n_slots, const T* d_table, const std::uint32_t* d_present, T missing, T* d_out,
                                       std::uint32_t* d_hit_mask = nullptr, std::uint64_t* d_stats = nullptr, std::uint32_t* d_err_flag = nullptr,
                                       void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_lookup_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, d_mask, n_blocks, key_lo, n_slots, d_table, d_present, missing, d_out, d_hit_mask, d_stats, d_err_flag, stream), "unfor_lookup_widths"); }
// ... with a uint8_t payload (for T = u8 the function above): d_out is the u8 key column of the grouped aggregates as it stands
template <typename T>
inline void unfor_lookup_u8_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                          const T* d_references, std::size_t reference_stride, const std::uint32_t* d_mask, std::size_t n_blocks,
                                          T key_lo, std::uint64_t n_slots, const std::uint8_t* d_table, const std::uint32_t* d_present,
                                          std::uint8_t missing, std::uint8_t* d_out, std::uint32_t* d_hit_mask = nullptr, std::uint64_t* d_stats = nullptr,
                                          std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_lookup_u8_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, d_mask, n_blocks, key_lo, n_slots, d_table, d_present, missing, d_out, d_hit_mask, d_stats, d_err_flag, stream), "unfor_lookup_u8_widths"); }
// ... and the u8 lookup fused with the grouped aggregate over two mixed-width columns of T with the same block count: d_result[g] (256
// slots, all written by every call) = count / sum / min / max of the values of the kept rows whose key hits a slot of d_table holding g,
// d_stats += {hits, kept rows that miss}; both columns get unfor_pack_widths' device checks, a block that fails either contributes nothing
template <typename T>
inline void unfor_aggregate_by_lookup_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                                    const T* d_references, std::size_t reference_stride, const std::uint8_t* d_key_widths,
                                                    const std::uint64_t* d_key_offsets, const T* d_keys, std::size_t keys_bytes,
                                                    const T* d_key_references, std::size_t key_reference_stride, const std::uint32_t* d_mask,
                                                    std::size_t n_blocks, T key_lo, std::uint64_t n_slots, const std::uint8_t* d_table,
                                                    const std::uint32_t* d_present, fl_block_aggregate* d_result, std::uint64_t* d_stats = nullptr,
                                                    std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_aggregate_by_lookup_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, d_key_widths, d_key_offsets, d_keys, keys_bytes, d_key_references, key_reference_stride, d_mask, n_blocks, key_lo, n_slots, d_table, d_present, d_result, d_stats, d_err_flag, stream), "unfor_aggregate_by_lookup_widths"); }
// ... and a predicate between two mixed-width columns of T with the same block count, a <op> b (signed: of the two's-complement values),
// chained the same way; both columns get unfor_pack_widths' device checks, a block that fails either keeps its mask words
template <typename T>
inline void unfor_compare_columns_widths_device(const std::uint8_t* d_a_widths, const std::uint64_t* d_a_offsets, const T* d_a_packed,
                                                std::size_t a_packed_bytes, const T* d_a_references, std::size_t a_reference_stride,
                                                const std::uint8_t* d_b_widths, const std::uint64_t* d_b_offsets, const T* d_b_packed,
                                                std::size_t b_packed_bytes, const T* d_b_references, std::size_t b_reference_stride, fl_cmp op,
                                                bool is_signed, fl_mask_combine combine, const std::uint32_t* d_mask_in, std::size_t n_blocks,
                                                std::uint32_t* d_mask, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_compare_columns_widths(d_a_widths, d_a_offsets, d_a_packed, a_packed_bytes, d_a_references, a_reference_stride, d_b_widths, d_b_offsets, d_b_packed, b_packed_bytes, d_b_references, b_reference_stride, (int)op, is_signed ? 1 : 0, (int)combine, d_mask_in, n_blocks, d_mask, d_err_flag, stream), "unfor_compare_columns_widths"); }
// selection mask -> where each block's kept values start in the compacted output (elements), and how many there are in all
inline void mask_offsets_device(const std::uint32_t* d_mask, std::size_t n_blocks, std::uint64_t* d_out_offsets, std::uint64_t* d_total = nullptr,
                                void* stream = nullptr)
{ detail::check(fl_mask_offsets(d_mask, n_blocks, d_out_offsets, d_total, stream), "mask_offsets"); }
// ... and the kept values themselves: unfor_pack_widths_device's output where the mask has a 1, compacted, in column order
template <typename T>
inline void unfor_select_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                       const T* d_references, std::size_t reference_stride, const std::uint32_t* d_mask,
                                       const std::uint64_t* d_out_offsets, T* d_out, std::size_t out_len, std::size_t n_blocks,
                                       std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_select_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, d_mask, d_out_offsets, d_out, out_len, n_blocks, d_err_flag, stream), "unfor_select_widths"); }
// ... or their count / sum / min / max per block, never materialised (d_mask == nullptr: every row); a block that fails the device checks
// gets the identity {0, 0, UINT64_MAX, 0}
template <typename T>
inline void unfor_aggregate_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                          const T* d_references, std::size_t reference_stride, const std::uint32_t* d_mask, std::size_t n_blocks,
                                          fl_block_aggregate* d_block_aggs, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_aggregate_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, d_mask, n_blocks, d_block_aggs, d_err_flag, stream), "unfor_aggregate_widths"); }
// unfor_aggregate_by over two mixed-width columns (value: T, key: u8) of the same block count; both columns get unfor_pack_widths' device
// checks, a block that fails either contributes nothing
template <typename T>
inline void unfor_aggregate_by_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                             const T* d_references, std::size_t reference_stride, const std::uint8_t* d_key_widths,
                                             const std::uint64_t* d_key_offsets, const std::uint8_t* d_keys, std::size_t keys_bytes,
                                             const std::uint8_t* d_key_references, std::size_t key_reference_stride, const std::uint32_t* d_mask,
                                             std::size_t n_blocks, fl_block_aggregate* d_result, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_aggregate_by_widths(d_widths, d_offsets, d_packed, packed_bytes, d_references, reference_stride, d_key_widths, d_key_offsets, d_keys, keys_bytes, d_key_references, key_reference_stride, d_mask, n_blocks, d_result, d_err_flag, stream), "unfor_aggregate_by_widths"); }
// unfor_aggregate_columns over two mixed-width columns of T with the same block count: count / sum / min / max per block of a * b, a + b or
// a - b; both columns get unfor_pack_widths' device checks, a block that fails either gets the identity
template <typename T>
inline void unfor_aggregate_columns_widths_device(fl_expr expr, const std::uint8_t* d_a_widths, const std::uint64_t* d_a_offsets, const T* d_a_packed,
                                                  std::size_t a_packed_bytes, const T* d_a_references, std::size_t a_reference_stride,
                                                  const std::uint8_t* d_b_widths, const std::uint64_t* d_b_offsets, const T* d_b_packed,
                                                  std::size_t b_packed_bytes, const T* d_b_references, std::size_t b_reference_stride,
                                                  const std::uint32_t* d_mask, std::size_t n_blocks, fl_block_aggregate* d_block_aggs,
                                                  std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_aggregate_columns_widths((int)expr, d_a_widths, d_a_offsets, d_a_packed, a_packed_bytes, d_a_references, a_reference_stride, d_b_widths, d_b_offsets, d_b_packed, b_packed_bytes, d_b_references, b_reference_stride, d_mask, n_blocks, d_block_aggs, d_err_flag, stream), "unfor_aggregate_columns_widths"); }
// unfor_aggregate_by_columns over three mixed-width columns with the same block count (a and b of T, the keys u8): d_result[g] (256 slots) =
// count / sum / min / max of a * b, a + b or a - b per key; all three columns get unfor_pack_widths' device checks, a block that fails any
// contributes nothing
template <typename T>
inline void unfor_aggregate_by_columns_widths_device(fl_expr expr, const std::uint8_t* d_a_widths, const std::uint64_t* d_a_offsets, const T* d_a_packed,
                                                     std::size_t a_packed_bytes, const T* d_a_references, std::size_t a_reference_stride,
                                                     const std::uint8_t* d_b_widths, const std::uint64_t* d_b_offsets, const T* d_b_packed,
                                                     std::size_t b_packed_bytes, const T* d_b_references, std::size_t b_reference_stride,
                                                     const std::uint8_t* d_key_widths, const std::uint64_t* d_key_offsets, const std::uint8_t* d_keys,
                                                     std::size_t keys_bytes, const std::uint8_t* d_key_references, std::size_t key_reference_stride,
                                                     const std::uint32_t* d_mask, std::size_t n_blocks, fl_block_aggregate* d_result,
                                                     std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unfor_aggregate_by_columns_widths((int)expr, d_a_widths, d_a_offsets, d_a_packed, a_packed_bytes, d_a_references, a_reference_stride, d_b_widths, d_b_offsets, d_b_packed, b_packed_bytes, d_b_references, b_reference_stride, d_key_widths, d_key_offsets, d_keys, keys_bytes, d_key_references, key_reference_stride, d_mask, n_blocks, d_result, d_err_flag, stream), "unfor_aggregate_by_columns_widths"); }
// per-block aggregates -> the column's: counts and sums added (wrapping), the smallest min, the largest max; no blocks: the identity
inline void aggregate_reduce_device(const fl_block_aggregate* d_block_aggs, std::size_t n_blocks, fl_block_aggregate* d_result, void* stream = nullptr)
{ detail::check(fl_aggregate_reduce(d_block_aggs, n_blocks, d_result, stream), "aggregate_reduce"); }
template <typename T>
inline void for_pack_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_in, const T* d_references,
                                   std::size_t reference_stride, T* d_packed, std::size_t packed_bytes, std::size_t n_blocks,
                                   std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::for_pack_widths(d_widths, d_offsets, d_in, d_references, reference_stride, d_packed, packed_bytes, n_blocks, d_err_flag, stream), "for_pack_widths"); }
template <typename T>
inline void undelta_pack_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_packed, std::size_t packed_bytes,
                                       const T* d_bases, T* d_out, std::size_t n_blocks, bool untranspose = false,
                                       std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{
    detail::check((untranspose ? detail::Abi<T>::undelta_pack_untranspose_widths : detail::Abi<T>::undelta_pack_widths)(
                      d_widths, d_offsets, d_packed, packed_bytes, d_bases, d_out, n_blocks, d_err_flag, stream), "undelta_pack_widths");
}
template <typename T>
inline void transpose_delta_pack_widths_device(const std::uint8_t* d_widths, const std::uint64_t* d_offsets, const T* d_in, const T* d_bases,
                                               T* d_packed, std::size_t packed_bytes, std::size_t n_blocks,
                                               std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::transpose_delta_pack_widths(d_widths, d_offsets, d_in, d_bases, d_packed, packed_bytes, n_blocks, d_err_flag, stream), "transpose_delta_pack_widths"); }
// An encoder's width choice between block_min_max and for_pack_widths: widths[b] = bit length of maxs[b] - mins[b] (extension).
template <typename T>
inline void for_widths_device(const T* d_mins, const T* d_maxs, std::size_t n_blocks, std::uint8_t* d_widths, void* stream = nullptr)
{ detail::check(detail::Abi<T>::for_widths(d_mins, d_maxs, n_blocks, d_widths, stream), "for_widths"); }
template <typename T>
inline void widths_to_offsets_device(const std::uint8_t* d_widths, std::size_t n_blocks, std::uint64_t* d_offsets,
                                     std::uint64_t* d_total_bytes = nullptr, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(fl_widths_to_offsets(sizeof(T) * 8, d_widths, n_blocks, d_offsets, d_total_bytes, d_err_flag, stream), "widths_to_offsets"); }

// Many small arrays (a columnar engine's chunks) in one launch: device arrays of device pointers / widths / block counts.
template <typename T>
inline void unpack_batch_device(const T* const* d_packed, T* const* d_out, const std::uint8_t* d_widths, const std::uint32_t* d_n_blocks,
                                std::size_t n_arrays, std::uint32_t max_blocks, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::unpack_batch(d_packed, d_out, d_widths, d_n_blocks, n_arrays, max_blocks, d_err_flag, stream), "unpack_batch"); }
template <typename T>
inline void pack_batch_device(const T* const* d_in, T* const* d_packed, const std::uint8_t* d_widths, const std::uint32_t* d_n_blocks,
                              std::size_t n_arrays, std::uint32_t max_blocks, std::uint32_t* d_err_flag = nullptr, void* stream = nullptr)
{ detail::check(detail::Abi<T>::pack_batch(d_in, d_packed, d_widths, d_n_blocks, n_arrays, max_blocks, d_err_flag, stream), "pack_batch"); }

}  // namespace fastlanes
