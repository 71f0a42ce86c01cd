// fl_tile_map.hpp -- the XCD-aware tile map shared by every kernel (workgroup -> tile) and its launch plan, as plain integer
// functions: used by the kernels and launchers through fl_kernels.hpp, and by a CPU test that compiles this header with a plain C++
// compiler (tests/test_tile_map_cpu.py: a permutation of the grid, XCD-contiguous, for every grid / window / rotate flag).
// No HIP dependency.
#pragma once
#include <stdint.h>

#ifndef FL_HD            // (also defined, identically, by fl_for_decide.hpp)
#if defined(__HIPCC__) || defined(__HIP__)
#define FL_HD __host__ __device__
#else
#define FL_HD
#endif
#endif

namespace fl {

// WINDOW_WHOLE = one window = the whole-column map (which kernel gets which window, and why: fl_dispatch.hpp)
constexpr int WINDOW_WHOLE = 31;

// The XCD-aware tile map shared by every kernel: workgroup b -> tile.  The grid is 8 * tiles_per_xcd workgroups (a multiple
// of 8; padding workgroups get tiles past the end and leave).  It is walked in windows of 2^window_shift tiles (the last one
// shorter; every window a multiple of 8 tiles): workgroups [first, first + span) serve window [first, first + span), and
// inside it workgroup r -- which runs on XCD r % 8 (observed dispatch order; used for speed only, results never depend on
// it) -- takes tile first + (r % 8) * span / 8 + r / 8, so XCD x owns one contiguous eighth of the window.  One window =
// rounds 1-3's map (XCD x owns one contiguous eighth of the whole column).  Why windows, and which kernel gets one: fl_dispatch.hpp.
// TILE_MAP_ROTATE (a flag next to the window shift; round 4, profiles/abmixed_rotate_r04.txt): inside an XCD's run the k-th row of
// 32 tiles is rotated by k tiles.  An XCD has 32 CUs and its workgroups go to them round-robin, so WITHOUT the rotation CU c is
// handed tiles c, c + 32, c + 64, ... of the run: if the data has a period that divides 32 tiles (BASELINE config 5: width[b] =
// 1 + b mod 32 -- 8 tiles) every CU sits at ONE phase of the pattern for the whole launch, some decoding only wide blocks, others only
// narrow ones.  Rotated, every CU walks through all phases: the ramp 0.798 -> 0.812 (what seeded-random widths get), random widths
// -0.2 %.  Uniform-width kernels have nothing to decorrelate and lose 0.2-1 % to it, so only the mixed-width kernels set it.
constexpr unsigned TILE_MAP_ROTATE = 0x80u;
// (U = the integer type the map is computed in: uint64_t in general; a kernel whose slot count is known to fit 31 bits may ask for
// uint32_t -- the same code in scalar registers half as wide)
template <typename U> FL_HD inline U rotate_rows_of_32(U r, U run, bool rotate)
{
    const U row = r >> 5;
    return (rotate && ((row + 1) << 5) <= run) ? ((row << 5) | ((r + row) & 31u)) : r;      // a short last row stays as it is
}
template <typename U = uint64_t> FL_HD inline U xcd_tile(unsigned b, U tiles_per_xcd, unsigned window_shift_and_flags)
{
    // a window is a multiple of 8 tiles: anything below 2^3 (a launcher that skipped plan_tiles / tile_window_shift) is taken as 2^3,
    // or several workgroups would map to one tile and others to none
    const unsigned window_shift = (window_shift_and_flags & 0x7fu) < 3u ? 3u : (window_shift_and_flags & 0x7fu);
    const bool rotate = (window_shift_and_flags & TILE_MAP_ROTATE) != 0;
    if (window_shift >= 32) return (U)(b & 7u) * tiles_per_xcd + rotate_rows_of_32<U>((U)(b >> 3), tiles_per_xcd, rotate);
    const unsigned first = (b >> window_shift) << window_shift;
    const unsigned r = b - first;
    const U left = tiles_per_xcd * 8 - first, full = (U)1 << window_shift;
    const U span = left < full ? left : full;
    return first + (U)(r & 7u) * (span >> 3) + rotate_rows_of_32<U>((U)(r >> 3), span >> 3, rotate);
}

// window_shift of a window of 2^log2_blocks blocks (>= WINDOW_WHOLE: the whole column) in tiles of `tile_blocks` blocks
inline unsigned window_shift_of(int log2_blocks, unsigned tile_blocks)
{
    if (log2_blocks >= WINDOW_WHOLE) return 63u;
    int tl = 0;
    while ((2u << tl) <= tile_blocks) ++tl;                  // floor(log2(tile_blocks))
    const int sh = log2_blocks - tl;
    return (unsigned)(sh < 3 ? 3 : sh);                      // a window is a multiple of 8 tiles
}

// THE LAUNCH PLAN of every kernel on the tile map: n_tiles tiles -> a grid of 8 XCD slots x tiles_per_xcd workgroups (padding
// workgroups exit at once), walked in windows of 2^window_shift tiles.  Fills the argument block's tile-map fields and returns the
// grid, or 0 past 2^31 workgroups (more than 2^33 blocks: no allocation on the card holds them), which a launcher refuses.
template <typename Args> inline unsigned plan_tiles(Args& a, uint64_t n_tiles, unsigned window_shift)
{
    a.tiles_per_xcd = (n_tiles + 7) / 8;
    a.window_shift = window_shift;
    return a.tiles_per_xcd * 8 > 0x7fffffffull ? 0u : (unsigned)(a.tiles_per_xcd * 8);
}

}  // namespace fl
