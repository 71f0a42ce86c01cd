"""CPU: the tile map every kernel launches through (fastlanes_amd/csrc/fl_tile_map.hpp: xcd_tile, rotate_rows_of_32,
window_shift_of, plan_tiles), compiled here for the host.  Correctness needs workgroup -> tile to be a permutation of
[0, 8 * tiles_per_xcd) for every grid, window and rotate flag -- a tile visited twice is invisible to every parity test (the same
bytes are written twice), a tile missed at an untested block count is invisible until somebody has that count -- and the map exists
to hand each XCD (workgroup id mod 8) one contiguous run of every window."""
import ctypes
import os

import numpy as np
import pytest

from cpu_support import ROOT, build_shim

ROTATE = 0x80
SHIFTS = list(range(14)) + [16, 20, 31, 32, 63]

SHIM = r"""
#include "fl_tile_map.hpp"
#include <stddef.h>
#include <atomic>
#include <mutex>
#include <thread>
#include <vector>
static_assert(fl::TILE_MAP_ROTATE == 0x80u && fl::WINDOW_WHOLE == 31, "");
template <typename U> static void tiles(unsigned b0, size_t n, uint64_t tpx, unsigned ws, uint64_t* out)
{
    for (size_t i = 0; i < n; ++i) out[i] = fl::xcd_tile<U>(b0 + (unsigned)i, (U)tpx, ws);
}
// 0: {xcd_tile(b) : b < 8 * tpx} == [0, 8 * tpx); else 1 + the first workgroup whose tile is out of range or already taken.
// `seen` holds a stamp per tile, so that one array serves many grids without being cleared.
template <typename U> static uint64_t not_a_permutation(uint64_t tpx, unsigned ws, std::vector<uint32_t>& seen, uint32_t stamp)
{
    const uint64_t slots = 8 * tpx;
    if (seen.size() < slots) seen.resize(slots, 0u);
    for (uint64_t b = 0; b < slots; ++b) {
        const uint64_t t = fl::xcd_tile<U>((unsigned)b, (U)tpx, ws);
        if (t >= slots || seen[t] == stamp) return 1 + b;
        seen[t] = stamp;
    }
    return 0;
}
// every (tiles_per_xcd, window shift | flags) pair of the two lists, the grids shared out over a few threads; 0, or 1 + the index
// (i_tpx * n_ws + i_ws) of a failing pair, its first bad workgroup in *bad_b
template <typename U> static uint64_t sweep(const uint64_t* tpx, size_t n_tpx, const unsigned* ws, size_t n_ws, uint64_t* bad_b)
{
    std::atomic<size_t> next{0};
    std::atomic<uint64_t> bad{0};
    std::mutex m;
    auto work = [&] {
        std::vector<uint32_t> seen;
        uint32_t stamp = 0;
        for (size_t i; (i = next.fetch_add(1)) < n_tpx && !bad.load();)
            for (size_t j = 0; j < n_ws; ++j)
                if (const uint64_t b = not_a_permutation<U>(tpx[i], ws[j], seen, ++stamp)) {
                    std::lock_guard<std::mutex> g(m);
                    if (!bad.load()) { bad = 1 + i * n_ws + j; *bad_b = b - 1; }
                    return;
                }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    std::vector<std::thread> pool;
    for (unsigned k = 1; k < (hw < 1 ? 1u : hw > 8 ? 8u : hw); ++k) pool.emplace_back(work);
    work();
    for (auto& th : pool) th.join();
    return bad.load();
}
struct Plan { uint64_t tiles_per_xcd; unsigned window_shift; };
extern "C" {
void tiles_u64(unsigned b0, size_t n, uint64_t tpx, unsigned ws, uint64_t* out) { tiles<uint64_t>(b0, n, tpx, ws, out); }
void tiles_u32(unsigned b0, size_t n, uint64_t tpx, unsigned ws, uint64_t* out) { tiles<uint32_t>(b0, n, tpx, ws, out); }
uint64_t sweep_u64(const uint64_t* tpx, size_t n_tpx, const unsigned* ws, size_t n_ws, uint64_t* bad_b) { return sweep<uint64_t>(tpx, n_tpx, ws, n_ws, bad_b); }
uint64_t sweep_u32(const uint64_t* tpx, size_t n_tpx, const unsigned* ws, size_t n_ws, uint64_t* bad_b) { return sweep<uint32_t>(tpx, n_tpx, ws, n_ws, bad_b); }
unsigned shift_of(int log2_blocks, unsigned tile_blocks) { return fl::window_shift_of(log2_blocks, tile_blocks); }
unsigned plan(uint64_t n_tiles, unsigned ws, uint64_t* tpx, unsigned* ws_out)
{
    Plan p{~0ull, ~0u};
    const unsigned grid = fl::plan_tiles(p, n_tiles, ws);
    *tpx = p.tiles_per_xcd;
    *ws_out = p.window_shift;
    return grid;
}
}
"""


@pytest.fixture(scope="module")
def tm(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "tile_map", SHIM, extra=("-pthread",))
    for u in ("u64", "u32"):
        getattr(lib, "tiles_" + u).argtypes = [ctypes.c_uint, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]
        getattr(lib, "tiles_" + u).restype = None
        getattr(lib, "sweep_" + u).argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        getattr(lib, "sweep_" + u).restype = ctypes.c_uint64
    lib.shift_of.argtypes = [ctypes.c_int, ctypes.c_uint]
    lib.shift_of.restype = ctypes.c_uint
    lib.plan.argtypes = [ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
    lib.plan.restype = ctypes.c_uint

    def tiles(u, tpx, ws, b0=0, n=None):
        n = 8 * tpx - b0 if n is None else n
        out = np.empty(n, dtype=np.uint64)
        getattr(lib, "tiles_" + u)(b0, n, tpx, ws, out.ctypes.data)
        return out
    lib.tiles = tiles

    def first_bad(u, tpx_list, ws_list):
        """None, or (tiles_per_xcd, window shift | flags, workgroup) of a grid that is not a permutation."""
        a = np.array(tpx_list, dtype=np.uint64)
        w = np.array(ws_list, dtype=np.uint32)
        b = ctypes.c_uint64()
        r = getattr(lib, "sweep_" + u)(a.ctypes.data, a.size, w.ctypes.data, w.size, ctypes.byref(b))
        return None if r == 0 else (int(a[(r - 1) // w.size]), int(w[(r - 1) % w.size]), b.value)
    lib.first_bad = first_bad
    return lib


def test_header_has_no_hip_dependency():
    text = open(os.path.join(ROOT, "fastlanes_amd", "csrc", "fl_tile_map.hpp")).read()
    assert "hip" not in text.lower().replace("__hipcc__", "").replace("__hip__", "").replace("no hip dependency", "")
    assert '#include "' not in text
    kernels = open(os.path.join(ROOT, "fastlanes_amd", "csrc", "fl_kernels.hpp")).read()
    assert '#include "fl_tile_map.hpp"' in kernels and "xcd_tile(unsigned b" not in kernels


def big_tpx():
    out = set()
    for k in range(1, 21):
        out |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    return sorted(x for x in out if x > 2000)


@pytest.mark.parametrize("u", ["u64", "u32"])
def test_every_grid_is_a_permutation(tm, u):
    """tiles_per_xcd 1..2000 and 2^k - 1, 2^k, 2^k + 1 up to 2^20; window shifts 0..13, 16, 20, 31, 32, 63; rotate off and on."""
    every = [ws | rot for ws in SHIFTS for rot in (0, ROTATE)]
    assert tm.first_bad(u, sorted(list(range(1, 2001)) + big_tpx(), reverse=True), every) is None


def test_shifts_below_3_behave_as_3(tm):
    for u in ("u64", "u32"):
        for tpx in (1, 2, 5, 33, 100, 257):
            for rot in (0, ROTATE):
                want = tm.tiles(u, tpx, 3 | rot)
                for ws in (0, 1, 2):
                    assert np.array_equal(tm.tiles(u, tpx, ws | rot), want), (u, tpx, ws, rot)


def test_u32_and_u64_maps_agree(tm):
    for tpx in (1, 7, 64, 1000, 4097, (1 << 17) + 1):
        for ws in (3, 9, 16, 63):
            for rot in (0, ROTATE):
                assert np.array_equal(tm.tiles("u32", tpx, ws | rot), tm.tiles("u64", tpx, ws | rot)), (tpx, ws, rot)


def expected_run(run, rotate):
    """Position inside an XCD's run of `run` tiles of its r-th workgroup: r, or -- rotated -- row k of 32 turned by k; a short last
    row stays as it is."""
    r = np.arange(run, dtype=np.uint64)
    if not rotate:
        return r
    k = r // 32
    full = (k + 1) * 32 <= run
    return np.where(full, k * 32 + (r % 32 + k) % 32, r)


@pytest.mark.parametrize("u", ["u64", "u32"])
def test_each_xcd_gets_one_contiguous_run_of_every_window(tm, u):
    """Inside a window of `span` tiles starting at `first`, the workgroups with b % 8 == x receive the tiles
    [first + x * span / 8, first + (x + 1) * span / 8), in order -- rotated: in order up to a turn inside each full row of 32."""
    for tpx in list(range(1, 140)) + [255, 256, 257, 1023, 1025, 4099]:
        slots = 8 * tpx
        for ws in SHIFTS if tpx < 140 else [s for s in SHIFTS if s >= 6]:      # (thousands of 8-tile windows say nothing new)
            eff = max(ws, 3)
            for rot in (0, ROTATE):
                t = tm.tiles(u, tpx, ws | rot)
                first = 0
                while first < slots:
                    span = slots - first if eff >= 32 else min(1 << eff, slots - first)
                    assert span % 8 == 0
                    run = span // 8
                    w = t[first:first + span].reshape(run, 8)                       # [r, x]
                    want = first + np.arange(8, dtype=np.uint64)[None, :] * run + expected_run(run, bool(rot))[:, None]
                    assert np.array_equal(w, want), (u, tpx, ws, bool(rot), first)
                    first += span


@pytest.mark.parametrize("rot", [0, ROTATE])
@pytest.mark.parametrize("ws", [13, 16, 20])
def test_large_grid_first_and_last_window(tm, ws, rot):
    """tiles_per_xcd = 2^28 - 1: 2^31 - 8 slots, the most plan_tiles grants, computed in uint32_t as the persistent kernels do.  The
    first window and the (short) last one, fully enumerated, map one-to-one onto their own tile ranges."""
    tpx = (1 << 28) - 1
    slots = 8 * tpx
    full = 1 << ws
    last = (slots - 1) // full * full
    assert slots - last == full - 8
    for u in ("u32", "u64"):
        for first, span in ((0, full), (last, slots - last)):
            t = tm.tiles(u, tpx, ws | rot, b0=first, n=span)
            assert np.array_equal(np.sort(t), np.arange(first, first + span, dtype=np.uint64)), (u, ws, rot, first)
    # the whole-column map at that size: XCD x's run starts at x * tiles_per_xcd
    t = tm.tiles("u32", tpx, 63 | rot, b0=0, n=8 * 64).reshape(64, 8)
    assert np.array_equal(t[0], np.arange(8, dtype=np.uint64) * tpx)
    assert np.array_equal(np.sort(t[:32, 3]), 3 * tpx + np.arange(32, dtype=np.uint64))


def test_window_shift_of(tm):
    """>= 3 always; 63 from WINDOW_WHOLE (31) up; otherwise log2_blocks - floor(log2(tile_blocks)) -- for the tile sizes the launchers
    use (32 blocks per workgroup; bpw * 4 blocks for 1..16 blocks per wavefront; 4 units for the bare stream) and a few others."""
    for tb in sorted({32, 4, 1, 2, 3, 6, 100, 128} | {4 * bpw for bpw in range(1, 17)}):
        fl2 = tb.bit_length() - 1
        for lg in range(-2, 70):
            got = tm.shift_of(lg, tb)
            assert got >= 3
            assert got == (63 if lg >= 31 else max(3, lg - fl2)), (lg, tb, got)


def test_plan_tiles(tm):
    """The grid is 8 * ceil(n_tiles / 8) workgroups, the window shift is passed through; 0 (refused) past 2^31 - 1 workgroups."""
    tpx, ws = ctypes.c_uint64(), ctypes.c_uint()
    for n in list(range(0, 70)) + [1000, 4097, (1 << 20) + 3, (1 << 31) - 9, (1 << 31) - 8]:
        for w in (3, 16, 63, 9 | ROTATE):
            grid = tm.plan(n, w, ctypes.byref(tpx), ctypes.byref(ws))
            assert grid == 8 * ((n + 7) // 8) and tpx.value == (n + 7) // 8 and ws.value == w, (n, w)
    for n in ((1 << 31) - 7, 1 << 31, (1 << 33) + 5, 1 << 40):
        assert tm.plan(n, 63, ctypes.byref(tpx), ctypes.byref(ws)) == 0
        assert tpx.value == (n + 7) // 8


def persistent_walk(g, grid, slots, n_tiles, tile_of):
    """The slot arithmetic of k_chain_columns_pipelined (fl_chain.hpp) for workgroup g: tile k + 1 is issued and tile k + 2's slot
    looked up before tile k is consumed; a slot >= slots, or a tile >= n_tiles, holds nothing.  -> (consumed tiles, issued tiles)."""
    def blocks_of(t):
        tile = int(tile_of[t]) if t < slots else n_tiles
        return tile if tile < n_tiles else None
    consumed, issued = [], []
    t1 = g + grid
    cur, nxt_meta = blocks_of(g), blocks_of(t1)
    issued.append(cur)
    while True:
        t2 = t1 + grid
        m2 = blocks_of(t2)
        nxt = nxt_meta
        issued.append(nxt)
        consumed.append(cur)
        if t1 >= slots:
            break
        cur, nxt_meta, t1 = nxt, m2, t2
    return consumed, issued


def test_persistent_walk_visits_every_tile_once(tm):
    """k_chain_columns_pipelined and its encode twin run a grid smaller than the slot count: workgroup g takes slots g, g + grid,
    g + 2 * grid, ... with a two-slot lookahead (persistent_walk models the loop; the kernel is not included).  Over all g every
    tile below n_tiles is consumed exactly once, whatever is issued is consumed by the same workgroup, and the lookahead past the last
    slot holds nothing -- for EVERY grid that is a multiple of 8 and <= slots, and a tile count that does or does not fill the
    last 8 slots."""
    for tpx in (1, 2, 3, 5, 8, 13, 32, 33):
        slots = 8 * tpx
        for ws in (3, 5, 8, 63, 5 | ROTATE, 63 | ROTATE):
            tile_of = tm.tiles("u32", tpx, ws)
            for n_tiles in (slots, slots - 7):
                for grid in range(8, slots + 1, 8):
                    visits = np.zeros(n_tiles, dtype=np.int64)
                    for g in range(grid):
                        consumed, issued = persistent_walk(g, grid, slots, n_tiles, tile_of)
                        assert issued == consumed + [None] and len(consumed) == len(range(g, slots, grid)), (tpx, ws, grid, g)
                        for tile in consumed:
                            if tile is not None:
                                visits[tile] += 1
                    assert (visits == 1).all(), (tpx, ws, n_tiles, grid)
