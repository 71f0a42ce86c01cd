// fl_pair.hip -- fl_column_pair_alloc / _free, the OPTIONAL allocation helper of include/fastlanes_amd.h, and what stands behind it:
// the memory-class probe, the 1-GiB chunk cache, the never-reused address arena, the chunk-arrangement search, the registry of live
// constructed pairs the launchers consult (fl_in_constructed_pair) and the PROBE layout choice.  The codec itself is in fl_capi.hip.
#include "../../include/fastlanes_amd.h"
#include "../../include/fastlanes_amd_internal.h"
#include "fl_host.hpp"
#include "fl_stream.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

namespace {

using namespace fl;

// classes[g] = 0, 1, 2 (or -1: no clean answer) for the n pieces of `piece` bytes at `base`: unpack_compare u32 W=20 reads the start of a
// representative piece and writes its 1/20 mask into piece g (at piece - min(piece / 2, 1 GiB)); the slow ones are of the
// representative's class (7.0 TB/s across classes, 6.05 TB/s inside one: profiles/exp_region_map_r03.txt, profiles/r06_vmm_placement.txt)
int probe_classes(char* base, size_t n, size_t piece, int* classes, hipStream_t s)
{
    constexpr unsigned PROBE_WIDTH = 20;
    const size_t probe_blocks = std::min<size_t>(2000000, piece / (128 * PROBE_WIDTH));
    const size_t mask_off = piece - std::min<size_t>(piece / 2, (size_t)1 << 30);
    for (size_t g = 0; g < n; ++g) classes[g] = -1;
    if (n == 0 || probe_blocks == 0) return FL_OK;
    int rc = FL_OK;
    // milliseconds of the probe reading piece gi and writing into piece gm: median of 3 after one untimed launch, under the whole-column
    // tile map the class map was characterised with (a windowed read stream interferes less with the thin write stream, which is the
    // point of the window and blunts the probe): an override for THIS THREAD's launches only -- concurrent calls of other threads keep
    // their own tile maps, and a concurrent fl_internal_set_kernel_policy is untouched
    auto probe_ms = [&](size_t gi, size_t gm, float& ms) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(base + gi * piece);
        uint32_t* mask = reinterpret_cast<uint32_t*>(base + gm * piece + mask_off);
        return median_ms(s, 1, 3, [&] {
            const int saved = fl::window_override_this_thread();
            fl::window_override_this_thread() = fl::WINDOW_WHOLE;
            const int r = fl_u32_unpack_compare(PROBE_WIDTH, src, FL_CMP_LT, 1u << (PROBE_WIDTH - 1), probe_blocks, mask, s);
            fl::window_override_this_thread() = saved;
            return r;
        }, &ms);
    };
    float threshold = 0.f;                                   // between the two levels, from the first representative
    std::vector<float> ms(n);
    for (int c = 0; c < 3 && rc == FL_OK; ++c) {
        size_t rep = 0;
        while (rep < n && classes[rep] != -1) ++rep;
        if (rep == n) break;
        classes[rep] = c;
        rc = fl_fill_random(base + rep * piece, probe_blocks * 128 * PROBE_WIDTH, 17 + rep, s);   // full-entropy probe input
        float slowest = 0.f, fastest = 1e30f;
        size_t others = 0;
        for (size_t g = 0; g < n && rc == FL_OK; ++g) {
            if (classes[g] != -1) continue;
            rc = probe_ms(rep, g, ms[g]);
            slowest = std::max(slowest, ms[g]);
            fastest = std::min(fastest, ms[g]);
            ++others;
        }
        if (rc != FL_OK || others == 0) break;
        if (threshold == 0.f) {
            if (slowest - fastest <= 0.05f * slowest) break;     // one level only: "all of my class" and "none of it" look the same
            threshold = 0.5f * (slowest + fastest);
        }
        for (size_t g = 0; g < n; ++g)
            if (classes[g] == -1 && ms[g] > threshold) classes[g] = c;
    }
    return rc;
}

// ---- fl_column_pair_alloc / _free ----------------------------------------------------------------------------------------------------
constexpr size_t PAIR_ALIGN = 256, PAIR_ZONE = (size_t)64 << 30, PAIR_MIB = (size_t)1 << 20, PAIR_GIB = (size_t)1 << 30;
constexpr size_t PAIR_INTERLEAVED_MIN = 8 * PAIR_GIB;       // below that a pair is a handful of chunks: nothing to arrange
inline size_t pair_pad(size_t b) { return (b + PAIR_ALIGN - 1) & ~(PAIR_ALIGN - 1); }


// Live FL_LAYOUT_INTERLEAVED pairs, for the launchers: a call whose buffers lie inside ONE constructed pair runs under the whole-column tile
// map whatever fl_window_table.inc says -- the table's windows (pack, the transposes, delta ...) are what plain allocations want (a window
// keeps the eight XCDs' reads inside one class of memory), while a constructed pair already has its input inside one class and wants the
// eight write positions spread over the output's rotation: w=31 never loses there and gains 1-3 % on every row the table windows
// (profiles/r06_window_matrix_constructed.txt; pack u32 W=7 0.821 -> 0.836, then 0.859 with the three-class output rotation).
// [lo, hi) per live pair under a mutex; the count lets a process without such pairs skip the lock (one relaxed load per call).
std::mutex g_live_mutex;
std::vector<std::pair<uintptr_t, uintptr_t>> g_live;
std::atomic<int> g_live_count{0};
void live_pair_add(const char* va, size_t bytes)
{
    const uintptr_t lo = reinterpret_cast<uintptr_t>(va);
    std::lock_guard<std::mutex> lock(g_live_mutex);
    g_live.emplace_back(lo, lo + bytes);
    g_live_count.store((int)g_live.size(), std::memory_order_relaxed);
}
void live_pair_remove(const char* va)
{
    const uintptr_t lo = reinterpret_cast<uintptr_t>(va);
    std::lock_guard<std::mutex> lock(g_live_mutex);
    g_live.erase(std::remove_if(g_live.begin(), g_live.end(), [&](const auto& r) { return r.first == lo; }), g_live.end());
    g_live_count.store((int)g_live.size(), std::memory_order_relaxed);
}

// A bounded cache of 1-GiB physical chunks (fl_internal_pair_chunk_cache: OFF unless a tool asks for it).  hipMemCreate costs ~30 ms per
// GiB, so a constructed pair costs seconds, nearly all of it creating chunks that are released again a moment later; a sweep that builds a
// pair per row keeps them instead.  Only the handles are kept -- every pool is classified afresh (2.4 ms per chunk), class labels do not
// carry over from one probe to the next.
constexpr int CACHE_DEVICES = 16;
std::vector<hipMemGenericAllocationHandle_t> g_chunk_cache[CACHE_DEVICES];
size_t g_chunk_cache_limit = 0;
std::atomic_flag g_chunk_cache_lock = ATOMIC_FLAG_INIT;
void recycle_chunk(hipMemGenericAllocationHandle_t h, int dev)
{
    bool kept = false;
    if (dev >= 0 && dev < CACHE_DEVICES) {
        while (g_chunk_cache_lock.test_and_set(std::memory_order_acquire)) {}
        if (g_chunk_cache[dev].size() < g_chunk_cache_limit) { g_chunk_cache[dev].push_back(h); kept = true; }
        g_chunk_cache_lock.clear(std::memory_order_release);
    }
    if (!kept) (void)hipMemRelease(h);
}
bool cached_chunk(int dev, hipMemGenericAllocationHandle_t& h)
{
    bool got = false;
    if (dev >= 0 && dev < CACHE_DEVICES) {
        while (g_chunk_cache_lock.test_and_set(std::memory_order_acquire)) {}
        if (!g_chunk_cache[dev].empty()) { h = g_chunk_cache[dev].back(); g_chunk_cache[dev].pop_back(); got = true; }
        g_chunk_cache_lock.clear(std::memory_order_release);
    }
    return got;
}

struct ColumnPair {
    void* bufs[3] = {nullptr, nullptr, nullptr};       // separate: in, aux, out; zoned: the slab only
    void *in = nullptr, *aux = nullptr, *out = nullptr;
    // FL_LAYOUT_INTERLEAVED: physical chunks (hipMemCreate) mapped into one reserved address range
    std::vector<hipMemGenericAllocationHandle_t> chunks;
    char* va = nullptr;
    size_t va_bytes = 0, chunk_bytes = 0, n_mapped = 0;
    int dev = -1;                                        // the device the chunks belong to
    char class_map[96] = {0};                            // 'A' 'B' 'C' '?' per mapped chunk (first 95), input first
    ColumnPair() = default;
    ColumnPair(const ColumnPair&) = delete;
    ColumnPair& operator=(const ColumnPair&) = delete;
    ~ColumnPair()
    {
        for (void* b : bufs)
            if (b) (void)hipFree(b);
        if (n_mapped) {                                  // hipFree waits for queued work, hipMemUnmap does not: wait as hipFree would
            int cur = -1;
            const bool switched = hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess;
            (void)hipDeviceSynchronize();
            if (switched) (void)hipSetDevice(cur);
        }
        for (size_t i = 0; i < n_mapped; ++i) (void)hipMemUnmap(va + i * chunk_bytes, chunk_bytes);
        for (auto h : chunks) recycle_chunk(h, dev);
        if (va) { live_pair_remove(va); (void)hipMemAddressFree(va, va_bytes); }
    }
};

// Address ranges for FL_LAYOUT_INTERLEAVED.  On this ROCm (7.2) an address range that held a mapping, was unmapped and is mapped AGAIN --
// even after hipMemAddressFree + hipMemAddressReserve -- keeps translating to the chunks it held FIRST (tools/exp_vmm remap,
// profiles/r06_vmm_placement.txt): kernels would silently read and write memory that is no longer ours.  So no range is ever used twice
// within a process: ranges are asked for at monotonically growing addresses of a private stretch of the address space (16 .. 112 TiB; a hint that collides with something mapped there just yields another address: enough for several hundred pairs -- a pair uses its own size plus its pool's, once; then hipErrorOutOfMemory), and
// whatever the runtime returns is checked against every range this library used before.
std::atomic<uintptr_t> g_va_next{(uintptr_t)0x100000000000ull};
constexpr uintptr_t VA_ARENA_END = (uintptr_t)0x700000000000ull;
std::atomic_flag g_va_lock = ATOMIC_FLAG_INIT;
std::vector<std::pair<uintptr_t, uintptr_t>> g_va_used;

hipError_t reserve_fresh_range(size_t bytes, char** out)
{
    std::vector<void*> rejected;
    hipError_t e = hipErrorOutOfMemory;
    *out = nullptr;
    for (int attempt = 0; attempt < 6 && !*out; ++attempt) {
        const uintptr_t span = ((bytes + PAIR_GIB - 1) & ~(PAIR_GIB - 1)) + PAIR_GIB;
        const uintptr_t hint = g_va_next.fetch_add(span, std::memory_order_relaxed);
        if (hint + span > VA_ARENA_END) { e = hipErrorOutOfMemory; break; }
        void* p = nullptr;
        e = hipMemAddressReserve(&p, bytes, 2 * PAIR_MIB, reinterpret_cast<void*>(hint), 0);
        if (e != hipSuccess) { (void)hipGetLastError(); continue; }
        const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + bytes;
        while (g_va_lock.test_and_set(std::memory_order_acquire)) {}
        bool used = false;
        for (const auto& r : g_va_used) used = used || (lo < r.second && r.first < hi);
        if (!used) g_va_used.emplace_back(lo, hi);
        g_va_lock.clear(std::memory_order_release);
        if (used) { rejected.push_back(p); e = hipErrorOutOfMemory; }    // held until the end so that the runtime offers another one
        else *out = static_cast<char*>(p);
    }
    for (void* p : rejected) (void)hipMemAddressFree(p, bytes);
    return *out ? hipSuccess : e;
}

// which chunks of a classified pool form the pair (profiles/r06_vmm_placement.txt, r06_vmm/vmm_ratio_*.txt, vmm_pos_*.txt; fractions of 8 TB/s):
//  * the input (+ aux) inside ONE class (reads spread over classes under the whole-column tile map: 0.80 where one class gives 0.84-0.86);
//  * the output over `out_classes` classes: the OTHER TWO for a write-dominated pair (u32 W=7 unpack: out BC 0.864-0.866, out ABC 0.860,
//    out AB 0.855, out B 0.80, out A 0.78), ALL THREE otherwise (pack u32 W=7: out ABC 0.859, out AB 0.85, out BC 0.84, out B 0.83;
//    transpose: ABC 0.880, BC 0.870-0.879; unpack u32 W=20: equal);
//  * arranged for the WRITE POSITIONS, not in fixed runs: under the whole-column tile map XCD x walks the x-th eighth of the output, all
//    eight at the same pace, so at progress t the eight positions are the chunks floor((x + t) * n_out / 8).  What the memory wants is
//    those eight spread evenly over the classes AT EVERY t.  A fixed run length resonates with the eighth's size for some column lengths
//    (runs of 2 GiB at 8 M blocks: seven of the eight positions in one class, 0.840 where a balanced arrangement gives 0.864; runs of 1 GiB
//    with three classes at 6.5 M blocks: 0.829 / 0.859), and so does any closed formula once a chunk straddles two eighths (n_out = 20: the
//    "k-th chunk of eighth x takes letter x + k" rule puts all eight positions into one class at t = 0 -- unpack u16 W=3 0.852 where runs of
//    two had 0.868).  So the arrangement is SEARCHED: cost = mean over 64 values of t of the eight positions' cubed class
//    counts (an even spread is cheapest), plus a large penalty per chunk a class does not have and a fee per chunk of a
//    class outside the rotation (the input's own class: in A | out A and B alternating is 0.855, out B alone 0.80; unclassified chunks
//    last); start = letters by the position of a chunk's centre, then single-chunk relabelling until nothing improves (n_out * 4 * 64 * 8
//    operations per sweep: microseconds).  Creation order (short class runs by nature: 0.854-0.861) when no class can hold the input.
void choose_chunks(const std::vector<int>& cls, size_t n_in, size_t n_out, int out_classes, std::vector<int>& order, size_t* kept_out = nullptr)
{
    if (kept_out) *kept_out = 0;
    const size_t n = cls.size();
    order.clear();
    if (out_classes != 2) out_classes = 3;
    std::vector<int> by[4];                                    // 0..2 = classes, 3 = unclassified
    for (size_t g = 0; g < n; ++g) by[cls[g] < 0 || cls[g] > 2 ? 3 : cls[g]].push_back((int)g);
    if (n_out == 0 || n_in + n_out > n) {                      // nothing to arrange / the pool is too small: as created, as far as it goes
        for (size_t g = 0; g < n_in + n_out && g < n; ++g) order.push_back((int)g);
        return;
    }
    constexpr int TS = 64;                                     // samples of the progress t
    // pos[t][x] = the chunk under XCD x's write position at progress (t + 0.5) / TS
    std::vector<unsigned> pos((size_t)TS * 8);
    for (int t = 0; t < TS; ++t)
        for (int x = 0; x < 8; ++x) {
            const double p = (x + (t + 0.5) / TS) * (double)n_out / 8.0;
            pos[(size_t)t * 8 + x] = (unsigned)std::min<double>((double)n_out - 1, p);
        }
    struct Plan { std::vector<int> label; double cost; size_t kept; };
    auto plan = [&](int c) {
        Plan P;
        size_t avail[4] = {by[0].size(), by[1].size(), by[2].size(), by[3].size()};
        avail[c] -= n_in;
        // cost = the mean over t of sum_k count_k^3 (8 positions: 4 + 4 + 0 costs 128, 8/3 each 57, all in one class 512) + a fee per
        // FRACTION of the output taken from outside the rotation.  The cube and 600 for the input's own class rank the layouts as measured
        // (unpack u32 W=7, input in A): out BC 128 (0.865) < ABC 257 (0.860) < AB 428 (0.855) < B alone 512 (0.80) < A alone 1112 (0.78);
        // with squares no fee ranks "in B | out four fifths A" behind "in A | out A and B alternating" AND keeps BC ahead of ABC.  Below
        // ~300 the search sprinkles chunks of the input's class into a balanced pool's output (one such chunk gains 288 / n_out by taking a
        // position out of a 4 + 4 split): measured -0.4 % at 150, -0.0 ... -0.4 % at 300 against 1000 (profiles/r06_exp_own_class_fee.txt);
        // above 768 "B alone" would beat "A and B alternating" where a class is missing.
        static const double own_class_fee = [] { const char* e = getenv("FL_INTERNAL_OWN_CLASS_FEE"); return e ? atof(e) : 600.0; }();   // A/B tools
        double fee[4] = {0, 0, 0, own_class_fee + 50.0};
        bool in_rotation[3], plentiful = true;
        for (int k = 0; k < 3; ++k) {
            in_rotation[k] = out_classes == 3 || k != c;
            if (in_rotation[k] && avail[k] * (size_t)out_classes < n_out + (size_t)out_classes - 1) plentiful = false;
        }
        // ... where the rotation's classes cannot cover the output evenly the input's class has to help, and half the fee ranks "the scarce
        // class + the input's class + the plentiful one, evenly" ahead of "two thirds in the plentiful class" (AB 0.855 against B alone 0.80)
        for (int k = 0; k < 3; ++k) fee[k] = in_rotation[k] ? 0.0 : plentiful ? own_class_fee : 0.5 * own_class_fee;
        const int S[3] = {(c + 1) % 3, (c + 2) % 3, c};
        P.label.assign(n_out, 0);
        for (size_t j = 0; j < n_out; ++j) {                   // start: by the position of the chunk's centre
            const double at = (j + 0.5) * 8.0 / (double)n_out;
            const size_t x = (size_t)at, k = (size_t)((at - (double)x) * (double)n_out / 8.0);
            P.label[j] = S[(x + k) % (size_t)out_classes];
        }
        auto cost_of = [&](const std::vector<int>& lab) {
            double cost = 0.0;
            size_t used[4] = {0, 0, 0, 0};
            for (int k : lab) { ++used[k]; cost += fee[k] / (double)n_out; }
            for (int k = 0; k < 4; ++k) if (used[k] > avail[k]) cost += 10000.0 * (double)(used[k] - avail[k]);
            for (int t = 0; t < TS; ++t) {
                double cnt[4] = {0, 0, 0, 0};
                for (int x = 0; x < 8; ++x) cnt[lab[pos[(size_t)t * 8 + x]]] += 1.0;
                for (int k = 0; k < 4; ++k) cost += cnt[k] * cnt[k] * cnt[k] / TS;
            }
            return cost;
        };
        P.cost = cost_of(P.label);
        for (int sweep = 0; sweep < 12; ++sweep) {
            bool improved = false;
            for (size_t j = 0; j < n_out; ++j) {
                const int was = P.label[j];
                int best = was;
                for (int k = 0; k < 4; ++k) {
                    if (k == was) continue;
                    P.label[j] = k;
                    const double cst = cost_of(P.label);
                    if (cst < P.cost - 1e-9) { P.cost = cst; best = k; }
                }
                P.label[j] = best;
                improved = improved || best != was;
            }
            if (!improved) break;
        }
        // "kept" = chunks of rotation classes, less what the class shares are out of balance by (the pool-growth criterion)
        size_t used[4] = {0, 0, 0, 0};
        for (int k : P.label) ++used[k];
        double off = 0.0;
        size_t outside = used[3];
        for (int k = 0; k < 3; ++k) {
            if (in_rotation[k]) off += std::max(0.0, std::fabs((double)used[k] - (double)n_out / out_classes) - 1.0);
            else outside += used[k];
        }
        const double kept = (double)n_out - (double)outside - off;
        P.kept = kept > 0.0 ? (size_t)kept : 0;
        for (int k = 0; k < 4; ++k) if (used[k] > avail[k]) P.kept = 0;      // cannot even be filled
        return P;
    };
    int best_c = -1;
    Plan best;
    for (int c = 0; c < 3; ++c) {
        if (by[c].size() < n_in) continue;
        Plan P = plan(c);
        if (best_c < 0 || P.cost < best.cost - 1e-9 || (std::fabs(P.cost - best.cost) <= 1e-9 && by[c].size() > by[best_c].size())) { best = std::move(P); best_c = c; }
    }
    if (best_c < 0) {                                           // no class can hold the input: as created
        for (size_t g = 0; g < n_in + n_out && g < n; ++g) order.push_back((int)g);
        return;
    }
    if (kept_out) *kept_out = best.kept;
    size_t next[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < n_in; ++i) order.push_back(by[best_c][next[best_c]++]);
    for (size_t j = 0; j < n_out; ++j) {
        int k = best.label[j];
        if (next[k] >= by[k].size()) {                          // (only if the penalty lost against the imbalance: any chunk that is left)
            k = -1;
            for (int q = 0; q < 4; ++q) if (next[q] < by[q].size() && (k < 0 || by[q].size() - next[q] > by[k].size() - next[k])) k = q;
            if (k < 0) break;
        }
        order.push_back(by[k][next[k]++]);
    }
}
}  // namespace

// at least two of a call's pointers inside one live constructed pair (its input and its output; widths[] / offsets[] / references may live anywhere)
bool fl::fl_in_constructed_pair(std::initializer_list<const void*> ptrs)
{
    if (g_live_count.load(std::memory_order_relaxed) == 0) return false;
    std::lock_guard<std::mutex> lock(g_live_mutex);
    for (const auto& [lo, hi] : g_live) {
        int inside = 0;
        for (const void* p : ptrs) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(p);
            inside += (a >= lo && a < hi);
        }
        if (inside >= 2) return true;
    }
    return false;
}

namespace {

// (one construction at a time per process: the class probe TIMES small kernels, and two threads probing at once -- on one device or on two
// that share nothing but this code -- would read each other's interference as class boundaries)
std::mutex g_construct_mutex;

hipError_t pair_alloc_interleaved(size_t in_bytes, size_t aux_bytes, size_t out_bytes, hipStream_t s, ColumnPair& p, int& rc)
{
    std::lock_guard<std::mutex> one_at_a_time(g_construct_mutex);
    rc = FL_OK;
    int dev = 0, vmm = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&vmm, hipDeviceAttributeVirtualMemoryManagementSupported, dev);
    if (e != hipSuccess) return e;
    if (!vmm) return hipErrorNotSupported;
    const size_t in_span = pair_pad(in_bytes) + pair_pad(aux_bytes), total = in_span + pair_pad(out_bytes);
    const size_t chunk = PAIR_GIB;        // the class probe reads a whole piece: 0.17 ms per GiB is cleanly binary, 256-MiB pieces (45 us) are not
    const size_t n_in = std::max<size_t>(1, (in_span + chunk - 1) / chunk), n_out = std::max<size_t>(1, (pair_pad(out_bytes) + chunk - 1) / chunk);
    // enough chunks that a third of them holds the input and the other two thirds hold half the output each -- and twice the pair, because
    // the classes come in clusters of 4 .. 16 chunks (profiles/r06_vmm_placement.txt): a pool of just the pair's size often lacks one class
    // ... and never less than 48 GiB of them: a small pair's pool would otherwise lie inside one or two clusters
    // (with the output rotating through all three classes the input's class carries n_in + n_out / 3 of them)
    const int out_classes = pair_pad(out_bytes) >= 3 * in_span ? 2 : 3;
    size_t n_pool = std::max(std::max(std::max(3 * n_in + (out_classes == 3 ? n_out : 0), (3 * n_out + 1) / 2), 2 * (n_in + n_out)), 48 * PAIR_GIB / chunk);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 3 * PAIR_GIB) n_pool = std::min(n_pool, (free_b - 2 * PAIR_GIB) / chunk);
    if (n_pool < n_in + n_out) return hipErrorOutOfMemory;
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    hipMemAccessDesc acc{};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    std::vector<hipMemGenericAllocationHandle_t> pool;
    auto drop_pool = [&] { for (auto h : pool) recycle_chunk(h, dev); pool.clear(); };
    p.dev = dev;
    const size_t pool_cap = free_b > 3 * PAIR_GIB ? (free_b - 2 * PAIR_GIB) / chunk : n_pool;
    std::vector<int> cls, order;
    // The pool GROWS while the arrangement it allows is poor: the classes come in clusters of 4 .. 32 chunks, so a pool of the first size
    // is sometimes two thirds one class (a box of round 6: in A x10 | out BAAAABBCAAABBAA -- Delta over a u8 column at 0.77 where a
    // balanced pool gives 0.80).  A round = more chunks (half as many again, three rounds at most, never beyond three times the pair or the free memory), ALL of
    // them classified again through a fresh scratch range (2.4 ms per chunk), the arrangement chosen again; "poor" = fewer than nine in
    // ten output positions got the class the rotation asks for.
    for (int round = 0;; ++round) {
        pool.reserve(n_pool);
        while (pool.size() < n_pool) {
            hipMemGenericAllocationHandle_t h;
            if (!cached_chunk(dev, h) && hipMemCreate(&h, chunk, &prop, 0) != hipSuccess) { (void)hipGetLastError(); break; }
            pool.push_back(h);
        }
        if (pool.size() < n_in + n_out) { drop_pool(); return hipErrorOutOfMemory; }
        // 1. every chunk's class, measured through a scratch address range (used once, never again)
        cls.assign(pool.size(), -1);
        char* scratch = nullptr;
        e = reserve_fresh_range(pool.size() * chunk, &scratch);
        if (e != hipSuccess) { drop_pool(); return e; }
        size_t mapped = 0;
        for (; mapped < pool.size() && e == hipSuccess; ++mapped) e = hipMemMap(scratch + mapped * chunk, chunk, 0, pool[mapped], 0);
        if (e != hipSuccess) --mapped;
        if (e == hipSuccess) e = hipMemSetAccess(scratch, pool.size() * chunk, &acc, 1);
        if (e == hipSuccess) rc = probe_classes(scratch, pool.size(), chunk, cls.data(), s);
        if (e == hipSuccess && rc == FL_OK) e = hipStreamSynchronize(s);
        for (size_t i = 0; i < mapped; ++i) (void)hipMemUnmap(scratch + i * chunk, chunk);
        (void)hipMemAddressFree(scratch, pool.size() * chunk);
        if (e != hipSuccess || rc != FL_OK) { drop_pool(); return e; }
        // 2. the pair's chunks in their final order
        size_t kept = 0;
        choose_chunks(cls, n_in, n_out, out_classes, order, &kept);
        const bool complete = order.size() == n_in + n_out;
        const size_t bigger = std::min(std::min(pool_cap, std::max<size_t>(3 * (n_in + n_out), 96)), pool.size() + std::max<size_t>(pool.size() / 2, 8));
        if ((complete && 10 * kept >= 9 * n_out) || round == 3 || pool.size() < n_pool || bigger <= pool.size()) {
            if (!complete) { drop_pool(); return hipErrorOutOfMemory; }
            break;
        }
        n_pool = bigger;
    }
    // ... mapped ONCE into the address range the caller gets
    std::vector<char> keep(pool.size(), 0);
    for (int g : order) keep[g] = 1;
    p.chunk_bytes = chunk;
    p.va_bytes = order.size() * chunk;
    e = reserve_fresh_range(p.va_bytes, &p.va);
    for (size_t i = 0; i < order.size() && e == hipSuccess; ++i) {
        e = hipMemMap(p.va + i * chunk, chunk, 0, pool[order[i]], 0);
        if (e == hipSuccess) p.n_mapped = i + 1;
    }
    if (e == hipSuccess) e = hipMemSetAccess(p.va, p.va_bytes, &acc, 1);
    for (size_t g = 0; g < pool.size(); ++g) {
        if (keep[g]) p.chunks.push_back(pool[g]);
        else recycle_chunk(pool[g], dev);
    }
    pool.clear();
    if (e != hipSuccess) return e;                         // the owner releases what was made
    for (size_t i = 0; i < order.size() && i + 1 < sizeof p.class_map; ++i) p.class_map[i] = cls[order[i]] < 0 ? '?' : (char)('A' + cls[order[i]]);
    p.in = p.va;
    p.aux = aux_bytes ? p.va + pair_pad(in_bytes) : nullptr;
    p.out = p.va + n_in * chunk;
    live_pair_add(p.va, p.va_bytes);
    return hipSuccess;
}

hipError_t pair_alloc(int layout, size_t in_bytes, size_t aux_bytes, size_t out_bytes, hipStream_t s, ColumnPair& p, int& rc)
{
    rc = FL_OK;
    if (layout == FL_LAYOUT_INTERLEAVED && pair_pad(in_bytes) + pair_pad(aux_bytes) + pair_pad(out_bytes) >= PAIR_INTERLEAVED_MIN)
        return pair_alloc_interleaved(in_bytes, aux_bytes, out_bytes, s, p, rc);
    if (layout == FL_LAYOUT_SEPARATE || layout == FL_LAYOUT_INTERLEAVED) {
        hipError_t e = hipMalloc(&p.bufs[0], in_bytes ? in_bytes : PAIR_ALIGN);
        if (e == hipSuccess && aux_bytes) e = hipMalloc(&p.bufs[1], aux_bytes);
        if (e == hipSuccess) e = hipMalloc(&p.bufs[2], out_bytes ? out_bytes : PAIR_ALIGN);
        if (e != hipSuccess) return e;
        p.in = p.bufs[0]; p.aux = p.bufs[1]; p.out = p.bufs[2];
        return hipSuccess;
    }
    // ONE allocation: the input (then aux) at offset 0, the output centred on the first 64-GiB multiple that leaves room for them
    const size_t in_end = pair_pad(in_bytes) + pair_pad(aux_bytes), half = pair_pad(out_bytes) / 2;
    size_t k = 1;
    while (k * PAIR_ZONE < half + in_end) {
        if (++k > 8) return hipErrorOutOfMemory;
    }
    const size_t out_off = (k * PAIR_ZONE - half) & ~(PAIR_ALIGN - 1);
    hipError_t e = hipMalloc(&p.bufs[0], out_off + pair_pad(out_bytes));
    if (e != hipSuccess) return e;
    char* base = static_cast<char*>(p.bufs[0]);
    p.in = base;
    p.aux = aux_bytes ? base + pair_pad(in_bytes) : nullptr;
    p.out = base + out_off;
    return hipSuccess;
}

// GB/s of a bare stream in -> out over the pair (median of 5 after 2 untimed), in the proportion of the two sizes; 0 = not measured
int pair_probe(const ColumnPair& p, size_t in_bytes, size_t aux_bytes, size_t out_bytes, hipStream_t s, double& gbps)
{
    const size_t big = in_bytes > out_bytes ? in_bytes : out_bytes;
    const size_t n_units = big / 4096;
    gbps = 0.0;
    if (n_units < 1024) return FL_OK;                           // too small to say anything
    auto unit = [&](size_t bytes) { size_t u = bytes / n_units & ~(size_t)15; return u > 4096 ? 4096 : u; };
    BareArgs a{static_cast<const char*>(p.in), static_cast<const char*>(p.aux), static_cast<char*>(p.out), n_units, 0,
               (unsigned)unit(in_bytes), aux_bytes >= n_units * 128 ? 128u : 0u, (unsigned)unit(out_bytes), 63u};
    if (a.out_unit == 0) return FL_OK;
    float ms = 0.f;
    const int rc = median_ms(s, 2, 5, [&] { return hip_status(launch_bare_stream(a, true, a.in_unit > a.out_unit ? 8 : 6, WINDOW_WHOLE, s)); }, &ms);
    if (rc != FL_OK) return rc;
    if (!(ms > 0.f)) return FL_OK;                              // a zero median: not measured
    gbps = (double)n_units * (a.in_unit + a.aux_unit + a.out_unit) / (ms * 1e6);
    return FL_OK;
}

// FL_LAYOUT_PROBE's rule (fl_internal_choose_layout): does candidate `cand`, measured at `gbps`, replace the pair kept so far (layout
// `kept`, -1 = none yet, measured at `best`)?  The first candidate is always kept; a later one must win by more than 1 %, ZONED by more
// than 2 % (it pins ~64 GiB).
bool replaces_kept(int cand, double gbps, int kept, double best)
{
    return kept < 0 || gbps > best * (cand == FL_LAYOUT_ZONED ? 1.02 : 1.01);
}
constexpr int PROBE_ORDER[3] = {FL_LAYOUT_INTERLEAVED, FL_LAYOUT_SEPARATE, FL_LAYOUT_ZONED};
}  // namespace

extern "C" {

int fl_internal_probe_memory_classes(void* slab, size_t slab_bytes, int* classes, void* stream)
{
    const size_t n_granules = slab_bytes / FL_INTERNAL_GRANULE_BYTES;
    if (n_granules == 0) return FL_OK;
    if (!slab || !classes) return FL_ERR_NULL;
    if (misaligned(slab)) return FL_ERR_ALIGN;
    return probe_classes(static_cast<char*>(slab), n_granules, FL_INTERNAL_GRANULE_BYTES, classes, static_cast<hipStream_t>(stream));
}

int fl_column_pair_alloc(size_t in_bytes, size_t aux_bytes, size_t out_bytes, int layout, void* stream, void** in, void** aux, void** out,
                         void** handle, int* layout_kept, uint32_t* probe_gbps)
{
    if (!in || !out || !handle || (aux_bytes && !aux)) return FL_ERR_NULL;
    if (layout < 0 || layout >= FL_LAYOUT_COUNT) return FL_ERR_INDEX;
    FL_DEVICE_TIER(stream);                                  // FL_CHECK_DEVICE=1: `stream` must belong to the current device (the memory will)
    hipStream_t s = static_cast<hipStream_t>(stream);
    *in = *out = *handle = nullptr;
    if (aux) *aux = nullptr;
    if (probe_gbps) for (int i = 0; i < FL_LAYOUT_COUNT; ++i) probe_gbps[i] = 0;
    std::unique_ptr<ColumnPair> kept;
    int kept_layout = -1;
    const size_t biggest = in_bytes > out_bytes ? in_bytes : out_bytes;
    if (layout == FL_LAYOUT_PROBE && biggest / 4096 < 1024) layout = FL_LAYOUT_SEPARATE;   // too small to time: nothing to choose
    if (layout != FL_LAYOUT_PROBE) {
        kept.reset(new (std::nothrow) ColumnPair);
        if (!kept) return hip_fail(hipErrorOutOfMemory);
        int rc = FL_OK;
        if (hipError_t e = pair_alloc(layout, in_bytes, aux_bytes, out_bytes, s, *kept, rc); e != hipSuccess || rc != FL_OK)
            return rc != FL_OK ? rc : hip_fail(e);
        kept_layout = layout;
    } else {
        // the candidates one after the other (one that cannot be allocated next to the pair already held is skipped): a bare stream of
        // the pair's read : write proportion is timed on each; replaces_kept() decides.  The contents of the buffers are whatever the
        // stream left there.
        double best = -1.0;
        const bool large = pair_pad(in_bytes) + pair_pad(aux_bytes) + pair_pad(out_bytes) >= PAIR_INTERLEAVED_MIN;
        for (int cand : PROBE_ORDER) {
            if (cand == FL_LAYOUT_INTERLEAVED && !large) continue;      // would be the SEPARATE candidate twice
            std::unique_ptr<ColumnPair> p(new (std::nothrow) ColumnPair);
            int prc = FL_OK;
            if (!p || pair_alloc(cand, in_bytes, aux_bytes, out_bytes, s, *p, prc) != hipSuccess || prc != FL_OK) { (void)hipGetLastError(); continue; }
            double gbps = 0.0;
            if (const int r = pair_probe(*p, in_bytes, aux_bytes, out_bytes, s, gbps); r != FL_OK) return r;
            if (probe_gbps) probe_gbps[cand] = (uint32_t)(gbps + 0.5);
            if (replaces_kept(cand, gbps, kept_layout, best)) { kept = std::move(p); best = gbps; kept_layout = cand; }
        }
        if (!kept) return hip_fail(hipErrorOutOfMemory);
    }
    *in = kept->in;
    if (aux) *aux = kept->aux;
    *out = kept->out;
    if (layout_kept) *layout_kept = kept_layout;
    *handle = kept.release();
    return FL_OK;
}

int fl_column_pair_free(void* handle)
{
    delete static_cast<ColumnPair*>(handle);
    return FL_OK;
}

size_t fl_internal_pair_chunk_cache(size_t max_chunks)
{
    std::vector<hipMemGenericAllocationHandle_t> drop;
    size_t held = 0;
    while (g_chunk_cache_lock.test_and_set(std::memory_order_acquire)) {}
    g_chunk_cache_limit = max_chunks;
    for (auto& c : g_chunk_cache) {
        while (c.size() > max_chunks) { drop.push_back(c.back()); c.pop_back(); }
        held += c.size();
    }
    g_chunk_cache_lock.clear(std::memory_order_release);
    for (auto h : drop) (void)hipMemRelease(h);
    return held;
}

size_t fl_internal_choose_chunks(const int* classes, size_t n_pool, size_t n_in, size_t n_out, int out_classes, int* order)
{
    if (!classes || !order || n_pool == 0) return 0;
    std::vector<int> cls(classes, classes + n_pool), chosen;
    choose_chunks(cls, n_in, n_out, out_classes, chosen);
    for (size_t i = 0; i < chosen.size(); ++i) order[i] = chosen[i];
    return chosen.size();
}

int fl_internal_choose_layout(const double* gbps)
{
    int kept = -1;
    double best = -1.0;
    for (int cand : PROBE_ORDER)
        if (gbps && gbps[cand] >= 0.0 && replaces_kept(cand, gbps[cand], kept, best)) { kept = cand; best = gbps[cand]; }
    return kept;
}

const char* fl_internal_column_pair_classes(const void* handle)
{
    return handle ? static_cast<const ColumnPair*>(handle)->class_map : "";
}

}  // extern "C"
