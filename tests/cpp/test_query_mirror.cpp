// One query of each storage form through the C++ mirror (include/fastlanes_amd.hpp), for all four element types, on the GPU: a FoR
// chain (encode, round trip, two chained predicates, select, aggregates, a grouped aggregate, a semi-join and a lookup, every step in its
// mixed-width form) and a Delta chain.  A column has 7 blocks of widths {0, 1, 3, T/2, T-1, T, 2}: the smallest shape that holds every
// width route.  THE REFERENCE FOR EVERY RESULT IS A PLAIN LOOP OVER THE ORIGINAL HOST VALUES in uint64_t arithmetic (wrapping as
// include/fastlanes_amd.h defines), never a second call into the library; every comparison is exact.  Every output buffer is filled with
// a sentinel first and has guard words behind it that must survive.  Needs a GPU at run time (exits 2 without one); built on CPU as a
// compile / link check.
//   g++ -std=c++17 -I include -I /opt/rocm/include tests/cpp/test_query_mirror.cpp -L fastlanes_amd -lfastlanes_amd -L /opt/rocm/lib -lamdhip64
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include "fastlanes_amd.hpp"

using namespace fastlanes;

static int failures = 0;
static const char* current_type = "";
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAIL %s %s:%d %s\n", current_type, __FILE__, __LINE__, #cond); ++failures; } } while (0)
#define HIP(call) do { if ((call) != hipSuccess) throw std::runtime_error("HIP runtime error: " #call); } while (0)

constexpr size_t N = 7;                    // blocks per column
constexpr size_t GUARD = 64;               // bytes behind every device buffer
constexpr unsigned char SENTINEL = 0xA5;

struct SplitMix64 {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
};

// n elements in HBM, sentinel-filled, with GUARD sentinel bytes behind them
template <typename U> struct Dev {
    U* p = nullptr; size_t n;
    explicit Dev(size_t n_) : n(n_)
    {
        HIP(hipMalloc((void**)&p, n * sizeof(U) + GUARD));
        HIP(hipMemset(p, SENTINEL, n * sizeof(U) + GUARD));
    }
    explicit Dev(const std::vector<U>& h) : Dev(h.size()) { if (n) HIP(hipMemcpy(p, h.data(), n * sizeof(U), hipMemcpyHostToDevice)); }
    ~Dev() { (void)hipFree(p); }
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    void zero() { HIP(hipMemset(p, 0, n * sizeof(U))); }
    // the contents; the guard behind them must be as it was
    std::vector<U> down() const
    {
        std::vector<unsigned char> raw(n * sizeof(U) + GUARD);
        HIP(hipMemcpy(raw.data(), p, raw.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < GUARD; ++i) if (raw[n * sizeof(U) + i] != SENTINEL) { EXPECT(!"guard bytes overwritten"); break; }
        std::vector<U> h(n);
        if (n) std::memcpy(h.data(), raw.data(), n * sizeof(U));
        return h;
    }
};

static bool same(const fl_block_aggregate& a, const fl_block_aggregate& b) { return a.count == b.count && a.sum == b.sum && a.min == b.min && a.max == b.max; }
static void fold(fl_block_aggregate& a, uint64_t x) { a.count += 1; a.sum += x; a.min = std::min(a.min, x); a.max = std::max(a.max, x); }
constexpr fl_block_aggregate IDENTITY = {0, 0, UINT64_MAX, 0};
static bool bit(const std::vector<uint32_t>& words, size_t i) { return (words[i / 32] >> (i % 32)) & 1u; }

template <typename T> constexpr uint64_t max_of() { return (uint64_t)(T)~(T)0; }
template <typename T> static T low_bits(unsigned w) { return w == 0 ? (T)0 : (T)(max_of<T>() >> (sizeof(T) * 8 - w)); }
template <typename T> static std::vector<uint8_t> widths_of(int order)
{
    const uint8_t TB = sizeof(T) * 8;
    if (order == 0) return {0, 1, 3, (uint8_t)(TB / 2), (uint8_t)(TB - 1), TB, 2};
    return {TB, 2, (uint8_t)(TB - 1), 0, 3, 1, (uint8_t)(TB / 2)};
}

// A FoR column: host values (block b = its reference + a random number masked to widths[b] bits, never wrapping, with both ends of the range
// present so that the encoder must find exactly widths[b]), encoded on the device through the mirror's mixed-width encoder chain
template <typename T> struct ForColumn {
    std::vector<T> values, mins;
    std::vector<uint8_t> widths;
    std::vector<uint64_t> offsets;
    uint64_t packed_bytes = 0;
    Dev<T> d_refs;
    Dev<uint8_t> d_widths;
    Dev<uint64_t> d_offsets;
    Dev<T>* d_packed = nullptr;
    ~ForColumn() { delete d_packed; }

    // forced: (block, reference) pairs that fix a block's reference (the chain puts narrow blocks across its predicates' bounds); the rest are random
    ForColumn(uint64_t seed, const std::vector<uint8_t>& w, const std::vector<std::pair<size_t, T>>& forced, Dev<uint32_t>& d_err, hipStream_t stream)
        : values(N * 1024), mins(N), widths(w), offsets(N), d_refs(N), d_widths(N), d_offsets(N)
    {
        SplitMix64 rng{seed};
        for (size_t b = 0; b < N; ++b) {
            const T m = low_bits<T>(w[b]);
            const uint64_t room = max_of<T>() - m;                                       // references 0 .. room do not wrap
            T ref = room == UINT64_MAX ? (T)rng.next() : (T)(rng.next() % (room + 1));
            for (const auto& f : forced) if (f.first == b) ref = f.second;
            for (size_t i = 0; i < 1024; ++i) values[b * 1024 + i] = (T)(ref + (T)(rng.next() & m));
            const size_t at = rng.next() % 1023;
            values[b * 1024 + at] = ref;
            values[b * 1024 + at + 1] = (T)(ref + m);
            mins[b] = ref;
            offsets[b] = packed_bytes;
            packed_bytes += 128u * w[b];
        }
        // encode: block_min_max -> for_widths -> widths_to_offsets -> for_pack_widths, references = the blocks' minima, stride 1
        Dev<T> d_values(values), d_maxs(N);
        Dev<uint64_t> d_total(1);
        BitPacking<T>::block_min_max_device(d_values.p, N, d_refs.p, d_maxs.p, stream);
        for_widths_device<T>(d_refs.p, d_maxs.p, N, d_widths.p, stream);
        widths_to_offsets_device<T>(d_widths.p, N, d_offsets.p, d_total.p, d_err.p, stream);
        HIP(hipStreamSynchronize(stream));
        std::vector<T> maxs(N);
        for (size_t b = 0; b < N; ++b) {
            T lo = values[b * 1024], hi = lo;
            for (size_t i = 1; i < 1024; ++i) { lo = std::min(lo, values[b * 1024 + i]); hi = std::max(hi, values[b * 1024 + i]); }
            EXPECT(lo == mins[b]);
            maxs[b] = hi;
            unsigned bits = 0;
            for (uint64_t d = (uint64_t)hi - lo; d; d >>= 1) ++bits;
            EXPECT(bits == w[b]);
        }
        EXPECT(d_refs.down() == mins);
        EXPECT(d_maxs.down() == maxs);
        EXPECT(d_widths.down() == widths);
        EXPECT(d_offsets.down() == offsets);
        EXPECT(d_total.down()[0] == packed_bytes);
        d_packed = new Dev<T>(packed_bytes / sizeof(T));
        for_pack_widths_device<T>(d_widths.p, d_offsets.p, d_values.p, d_refs.p, 1, d_packed->p, packed_bytes, N, d_err.p, stream);
        HIP(hipStreamSynchronize(stream));
        (void)d_values.down();                                                           // the guards of the encoder's input
    }
};

template <typename T> static void for_chain(hipStream_t side)
{
    constexpr uint64_t MAXT = max_of<T>();
    constexpr size_t TB = sizeof(T) * 8, LANES = 1024 / TB;
    const T hi = (T)(MAXT / 4), lo = (T)(MAXT - MAXT / 4);                               // lo > hi: the cyclic interval [lo, MAXT] + [0, hi]
    const T key_lo = (T)(hi - 10);
    const uint64_t n_slots = TB == 8 ? 200 : 3000;                                       // above 2048 bits: probed in device memory
    Dev<uint32_t> d_err(1);
    d_err.zero();

    // 1. encode (a on the side stream).  a's width-1 block lies across lo and its width-3 block across hi; b's width-0 and width-3 blocks sit
    //    in the join window of steps 10 and 11, its width-(T-1) block above a's width-3 block and its width-1 block above everything, so that
    //    the chained mask keeps whole blocks, parts of blocks and nothing
    ForColumn<T> a(0xA11CE + TB, widths_of<T>(0), {{1, (T)(lo - 1)}, {2, (T)(hi - 3)}}, d_err, side);
    ForColumn<T> b(0xB0B + TB, widths_of<T>(1), {{1, (T)(lo - 1)}, {2, (T)(MAXT / 2)}, {3, (T)(hi + 20)}, {4, (T)(hi - 5)}, {5, (T)(MAXT - 1)}}, d_err, nullptr);
    ForColumn<uint8_t> k(0xCAFE + TB, widths_of<uint8_t>(0), {}, d_err, nullptr);

    // 2. round trip
    {
        Dev<T> d_out(N * 1024);
        unfor_pack_widths_device<T>(a.d_widths.p, a.d_offsets.p, a.d_packed->p, a.packed_bytes, a.d_refs.p, 1, d_out.p, N, d_err.p);
        EXPECT(d_out.down() == a.values);
        unfor_pack_widths_device<T>(b.d_widths.p, b.d_offsets.p, b.d_packed->p, b.packed_bytes, b.d_refs.p, 1, d_out.p, N, d_err.p);
        EXPECT(d_out.down() == b.values);
    }

    // 3. filter: a in the cyclic interval [lo, hi], a new mask
    Dev<uint32_t> d_mask(N * 32);
    std::vector<uint32_t> mask(N * 32, 0u);
    unfor_compare_range_widths_device<T>(a.d_widths.p, a.d_offsets.p, a.d_packed->p, a.packed_bytes, a.d_refs.p, 1, lo, hi, FL_MASK_NEW, nullptr, N, d_mask.p,
                                         d_err.p);
    for (size_t i = 0; i < N * 1024; ++i)
        if ((((uint64_t)a.values[i] - lo) & MAXT) <= (((uint64_t)hi - lo) & MAXT)) mask[i / 32] |= 1u << (i % 32);
    EXPECT(d_mask.down() == mask);

    // 4. chain: AND a < b (unsigned), in place
    unfor_compare_columns_widths_device<T>(a.d_widths.p, a.d_offsets.p, a.d_packed->p, a.packed_bytes, a.d_refs.p, 1, b.d_widths.p, b.d_offsets.p, b.d_packed->p,
                                           b.packed_bytes, b.d_refs.p, 1, FL_CMP_LT, false, FL_MASK_AND, d_mask.p, N, d_mask.p, d_err.p);
    for (size_t i = 0; i < N * 1024; ++i)
        if (!(a.values[i] < b.values[i])) mask[i / 32] &= ~(1u << (i % 32));
    EXPECT(d_mask.down() == mask);

    // 5. where each block's kept rows go
    std::vector<uint64_t> out_offsets(N);
    uint64_t total = 0;
    for (size_t blk = 0; blk < N; ++blk) {
        out_offsets[blk] = total;
        for (size_t i = 0; i < 1024; ++i) total += bit(mask, blk * 1024 + i);
    }
    EXPECT(total > 0 && total < N * 1024);
    Dev<uint64_t> d_out_offsets(N), d_total(1);
    mask_offsets_device(d_mask.p, N, d_out_offsets.p, d_total.p);
    EXPECT(d_out_offsets.down() == out_offsets);
    EXPECT(d_total.down()[0] == total);

    // 6. the kept rows of a, compacted
    {
        std::vector<T> kept;
        for (size_t i = 0; i < N * 1024; ++i) if (bit(mask, i)) kept.push_back(a.values[i]);
        Dev<T> d_kept(total);
        unfor_select_widths_device<T>(a.d_widths.p, a.d_offsets.p, a.d_packed->p, a.packed_bytes, a.d_refs.p, 1, d_mask.p, d_out_offsets.p, d_kept.p, total, N,
                                      d_err.p);
        EXPECT(d_kept.down() == kept);
    }

    // 7. COUNT / SUM / MIN / MAX of the kept rows of b per block, then of the column: read through the struct's fields
    {
        std::vector<fl_block_aggregate> want(N, IDENTITY);
        fl_block_aggregate all = IDENTITY;
        for (size_t i = 0; i < N * 1024; ++i) if (bit(mask, i)) { fold(want[i / 1024], b.values[i]); fold(all, b.values[i]); }
        Dev<fl_block_aggregate> d_aggs(N), d_result(1);
        unfor_aggregate_widths_device<T>(b.d_widths.p, b.d_offsets.p, b.d_packed->p, b.packed_bytes, b.d_refs.p, 1, d_mask.p, N, d_aggs.p, d_err.p);
        aggregate_reduce_device(d_aggs.p, N, d_result.p);
        const std::vector<fl_block_aggregate> got = d_aggs.down();
        for (size_t blk = 0; blk < N; ++blk) EXPECT(same(got[blk], want[blk]));
        const fl_block_aggregate r = d_result.down()[0];
        EXPECT(r.count == total && r.count == all.count);
        EXPECT(r.sum == all.sum);
        EXPECT(r.min == all.min);
        EXPECT(r.max == all.max);
    }

    // 8. the same of a - b (not commutative; a < b on every kept row, so every difference is a two's-complement pattern above 2^63 ...) and, with
    //    no mask, of every row (... here both signs occur)
    for (int masked = 1; masked >= 0; --masked) {
        std::vector<fl_block_aggregate> want(N, IDENTITY);
        fl_block_aggregate all = IDENTITY;
        for (size_t i = 0; i < N * 1024; ++i)
            if (!masked || bit(mask, i)) { const uint64_t x = (uint64_t)a.values[i] - (uint64_t)b.values[i]; fold(want[i / 1024], x); fold(all, x); }
        Dev<fl_block_aggregate> d_aggs(N), d_result(1);
        unfor_aggregate_columns_widths_device<T>(FL_EXPR_SUB, a.d_widths.p, a.d_offsets.p, a.d_packed->p, a.packed_bytes, a.d_refs.p, 1, b.d_widths.p, b.d_offsets.p,
                                                 b.d_packed->p, b.packed_bytes, b.d_refs.p, 1, masked ? d_mask.p : nullptr, N, d_aggs.p, d_err.p);
        aggregate_reduce_device(d_aggs.p, N, d_result.p);
        const std::vector<fl_block_aggregate> got = d_aggs.down();
        for (size_t blk = 0; blk < N; ++blk) EXPECT(same(got[blk], want[blk]));
        const fl_block_aggregate r = d_result.down()[0];
        EXPECT(r.count == all.count && r.sum == all.sum && r.min == all.min && r.max == all.max);
    }

    // 9. the kept rows of a grouped by the u8 key column: all 256 slots
    {
        std::vector<fl_block_aggregate> want(256, IDENTITY);
        for (size_t i = 0; i < N * 1024; ++i) if (bit(mask, i)) fold(want[k.values[i]], a.values[i]);
        Dev<fl_block_aggregate> d_groups(256);
        unfor_aggregate_by_widths_device<T>(a.d_widths.p, a.d_offsets.p, a.d_packed->p, a.packed_bytes, a.d_refs.p, 1, k.d_widths.p, k.d_offsets.p, k.d_packed->p,
                                            k.packed_bytes, k.d_refs.p, 1, d_mask.p, N, d_groups.p, d_err.p);
        const std::vector<fl_block_aggregate> got = d_groups.down();
        size_t groups = 0;
        for (size_t g = 0; g < 256; ++g) { EXPECT(same(got[g], want[g])); groups += want[g].count != 0; }
        EXPECT(groups > 16);
    }

    // 10. the semi-join: the member set of b's values inside the window, then a IN (that set)
    std::vector<uint32_t> set_words((n_slots + 31) / 32, 0u);
    {
        std::vector<uint64_t> stats(2, 0);
        for (size_t i = 0; i < N * 1024; ++i) {
            const uint64_t j = ((uint64_t)b.values[i] - key_lo) & MAXT;
            if (j < n_slots) { set_words[j / 32] |= 1u << (j % 32); ++stats[0]; } else ++stats[1];
        }
        Dev<uint32_t> d_set(set_words.size()), d_in(N * 32);
        Dev<uint64_t> d_stats(2);
        d_set.zero();
        d_stats.zero();
        unfor_set_build_widths_device<T>(b.d_widths.p, b.d_offsets.p, b.d_packed->p, b.packed_bytes, b.d_refs.p, 1, nullptr, N, key_lo, n_slots, d_set.p, d_stats.p,
                                         d_err.p);
        EXPECT(d_set.down() == set_words);
        EXPECT(d_stats.down() == stats);
        EXPECT(stats[0] >= 2048 && stats[1] > 0);
        std::vector<uint32_t> in(N * 32, 0u);
        size_t members = 0;
        for (size_t i = 0; i < N * 1024; ++i) {
            const uint64_t j = ((uint64_t)a.values[i] - key_lo) & MAXT;
            if (j < n_slots && bit(set_words, j)) { in[i / 32] |= 1u << (i % 32); ++members; }
        }
        unfor_compare_in_widths_device<T>(a.d_widths.p, a.d_offsets.p, a.d_packed->p, a.packed_bytes, a.d_refs.p, 1, key_lo, n_slots, d_set.p, false, FL_MASK_NEW,
                                          nullptr, N, d_in.p, d_err.p);
        EXPECT(d_in.down() == in);
        EXPECT(members > 0 && members < N * 1024);
    }

    // 11. a as a join key into a table over the same window, every third slot absent: the payload column (a full-width packed block is its
    //     1024 values permuted: bitpacking.rs), the hits and the counts
    {
        std::vector<T> table(n_slots);
        std::vector<uint32_t> present((n_slots + 31) / 32, 0u);
        for (uint64_t j = 0; j < n_slots; ++j) { table[j] = (T)(j * 7 + 1); if (j % 3) present[j / 32] |= 1u << (j % 32); }
        const T missing = (T)(MAXT - 2);
        std::vector<T> want(N * 1024);
        std::vector<uint32_t> hits(N * 32, 0u);
        std::vector<uint64_t> stats(2, 0);
        for (size_t blk = 0; blk < N; ++blk)
            for (size_t row = 0; row < TB; ++row)
                for (size_t lane = 0; lane < LANES; ++lane) {
                    const size_t i = blk * 1024 + FL_ORDER[row / 8] * 16 + (row % 8) * 128 + lane;
                    const uint64_t j = ((uint64_t)a.values[i] - key_lo) & MAXT;
                    const bool hit = bit(mask, i) && j < n_slots && bit(present, j);
                    want[blk * 1024 + LANES * row + lane] = hit ? table[j] : missing;
                    if (hit) hits[i / 32] |= 1u << (i % 32);
                    stats[0] += hit;
                    stats[1] += bit(mask, i) && !hit;
                }
        Dev<T> d_table(table), d_payload(N * 1024);
        Dev<uint32_t> d_present(present), d_hits(N * 32);
        Dev<uint64_t> d_stats(2);
        d_stats.zero();
        unfor_lookup_widths_device<T>(a.d_widths.p, a.d_offsets.p, a.d_packed->p, a.packed_bytes, a.d_refs.p, 1, d_mask.p, N, key_lo, n_slots, d_table.p, d_present.p,
                                      missing, d_payload.p, d_hits.p, d_stats.p, d_err.p);
        EXPECT(d_payload.down() == want);
        EXPECT(d_hits.down() == hits);
        EXPECT(d_stats.down() == stats);
        EXPECT(stats[0] + stats[1] == total && stats[0] > 0 && stats[1] > 0);
    }
    EXPECT(d_mask.down() == mask);                                                       // nothing behind step 4 wrote the mask
    EXPECT(d_err.down()[0] == 0u);
}

template <typename T> static void delta_chain(hipStream_t side)
{
    constexpr uint64_t MAXT = max_of<T>();
    constexpr size_t TB = sizeof(T) * 8, LANES = 1024 / TB;
    SplitMix64 rng{0xDE17A + TB};
    std::vector<T> values(N * 1024), bases(N * LANES);
    for (T& v : values) v = (T)rng.next();
    for (T& v : bases) v = (T)rng.next();
    const std::vector<uint8_t> widths(N, (uint8_t)TB);                                   // width T holds any values against any bases
    const uint64_t packed_bytes = N * 128 * TB;
    std::vector<uint64_t> offsets(N);
    for (size_t b = 0; b < N; ++b) offsets[b] = b * 128 * TB;
    Dev<uint32_t> d_err(1);
    d_err.zero();
    Dev<T> d_values(values), d_bases(bases), d_packed(N * 1024), d_out(N * 1024), d_transposed(N * 1024);
    Dev<uint8_t> d_widths(widths);
    Dev<uint64_t> d_offsets(N);
    widths_to_offsets_device<T>(d_widths.p, N, d_offsets.p, nullptr, d_err.p);
    EXPECT(d_offsets.down() == offsets);

    // 1. - 3. encode from row order; decode straight to row order, and to transposed order followed by the untranspose
    transpose_delta_pack_widths_device<T>(d_widths.p, d_offsets.p, d_values.p, d_bases.p, d_packed.p, packed_bytes, N, d_err.p);
    undelta_pack_widths_device<T>(d_widths.p, d_offsets.p, d_packed.p, packed_bytes, d_bases.p, d_out.p, N, true, d_err.p, side);
    HIP(hipStreamSynchronize(side));
    EXPECT(d_out.down() == values);
    undelta_pack_widths_device<T>(d_widths.p, d_offsets.p, d_packed.p, packed_bytes, d_bases.p, d_transposed.p, N, false, d_err.p);
    HIP(hipMemset(d_out.p, SENTINEL, N * 1024 * sizeof(T)));
    Transpose<T>::untranspose_device(d_transposed.p, d_out.p, N);
    EXPECT(d_out.down() == values);
    const std::vector<T> transposed = d_transposed.down();
    for (size_t i = 0; i < N * 1024; i += 41) EXPECT(transposed[i] == values[i / 1024 * 1024 + transpose(i % 1024)]);

    // 4. an interval over the values in row order
    const T lo = (T)(MAXT / 8), hi = (T)(MAXT / 2);
    std::vector<uint32_t> mask(N * 32, 0u);
    std::vector<uint64_t> out_offsets(N);
    std::vector<fl_block_aggregate> aggs(N, IDENTITY);
    std::vector<T> kept;
    for (size_t i = 0; i < N * 1024; ++i) {
        if (i % 1024 == 0) out_offsets[i / 1024] = kept.size();
        if ((((uint64_t)values[i] - lo) & MAXT) <= (((uint64_t)hi - lo) & MAXT)) {
            mask[i / 32] |= 1u << (i % 32);
            fold(aggs[i / 1024], values[i]);
            kept.push_back(values[i]);
        }
    }
    EXPECT(!kept.empty() && kept.size() < N * 1024);
    Dev<uint32_t> d_mask(N * 32);
    undelta_compare_range_widths_device<T>(d_widths.p, d_offsets.p, d_packed.p, packed_bytes, d_bases.p, lo, hi, FL_MASK_NEW, nullptr, N, d_mask.p, d_err.p);
    EXPECT(d_mask.down() == mask);

    // 5. the aggregate and the rows that mask keeps
    Dev<fl_block_aggregate> d_aggs(N);
    undelta_aggregate_widths_device<T>(d_widths.p, d_offsets.p, d_packed.p, packed_bytes, d_bases.p, d_mask.p, N, d_aggs.p, d_err.p);
    const std::vector<fl_block_aggregate> got = d_aggs.down();
    for (size_t b = 0; b < N; ++b) EXPECT(same(got[b], aggs[b]));
    Dev<uint64_t> d_out_offsets(N), d_total(1);
    mask_offsets_device(d_mask.p, N, d_out_offsets.p, d_total.p);
    EXPECT(d_out_offsets.down() == out_offsets);
    EXPECT(d_total.down()[0] == kept.size());
    Dev<T> d_kept(kept.size());
    undelta_select_widths_device<T>(d_widths.p, d_offsets.p, d_packed.p, packed_bytes, d_bases.p, d_mask.p, d_out_offsets.p, d_kept.p, kept.size(), N, d_err.p);
    EXPECT(d_kept.down() == kept);
    EXPECT(d_err.down()[0] == 0u);
    (void)d_values.down();
    (void)d_bases.down();
    (void)d_packed.down();
}

template <typename T> static void run(const char* name, hipStream_t side)
{
    current_type = name;
    for_chain<T>(side);
    delta_chain<T>(side);
    HIP(hipDeviceSynchronize());
}

int main()
{
    try {
        int devices = 0;
        if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0) throw std::runtime_error("HIP runtime error: no device");
        hipStream_t side = nullptr;
        HIP(hipStreamCreate(&side));
        run<uint8_t>("u8", side);
        run<uint16_t>("u16", side);
        run<uint32_t>("u32", side);
        run<uint64_t>("u64", side);
        HIP(hipStreamDestroy(side));
    } catch (const std::exception& e) {
        std::printf("EXCEPTION %s\n", e.what());
        return 2;
    }
    std::printf(failures ? "FAILED (%d)\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
