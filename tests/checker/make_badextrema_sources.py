#!/usr/bin/env python3
"""Makes the KNOWN-BAD sources of `make -C fastlanes_amd/csrc BADEXTREMA=1` (-> fastlanes_amd/libfastlanes_amd_badextrema.so): a copy
of the library's sources with ten defects in the kernels that take a minimum, a maximum or a sum.  Test scaffolding:
the product headers carry none of this.

    python tests/checker/make_badextrema_sources.py <csrc dir> <output dir>

Each defect changes ARITHMETIC only -- never an address, a bound, a load or store or control flow that guards memory -- and changes a
result only where ONE element decides it.  Each is also narrowed until the suite's random-data tests cannot see it (a masked-off row
that wins the minimum at any width shows at once in test_gpu_aggregate.py: a narrow block under a sparse mask is full of rows one
below the kept one); what is left is what only tests/extrema_data.py's columns reach (tests/test_gpu_extrema.py,
profiles/extrema_known_bad.txt):
1. block_min_max (fl_consume.hpp: k_block_min_max), u8: element 11 of the cell in row 5, column 3 -- index 699 of the block -- is left
   out of the maximum.  A random u8 block holds its maximum about 4 times over.
2. unfor_aggregate / unfor_aggregate_widths (fl_aggregate.hpp: aggregate_lds_image), u16 at W >= 15: a masked-off row still wins the
   minimum when it is exactly one below the lane's minimum so far -- for the second element of the lane's first cell, between two kept
   elements.  Random 15-bit neighbours differ by one once in 2^15 pairs.
3. the same function, u64 at W >= 56: the comparison for the maximum ignores bit 32 when the two values agree in bits 33..63.  Random
   56-bit values never do.
4. for_widths (fl_scan.hpp: k_for_widths): a span of exactly 2^k, k >= 17, gets k bits instead of k + 1.  The encoder-chain test masks
   its values to k bits; random pairs of u32 / u64 give a power of two once in 2^27.
The expression and grouped aggregates (tests/expr_extrema_data.py, tests/test_gpu_expr_extrema.py, tests/test_gpu_group_extrema.py,
profiles/expr_extrema_known_bad.txt), narrowed in the same way against their own older tests:
5. unfor_aggregate_columns (fl_aggregate_columns.hpp: expr_lds_image), u16 a + b with column b at W >= 15: a masked-off row wins the
   minimum when it is exactly one below the lane's minimum so far -- the second element of the lane's first cell between two kept ones.
6. expr_lds_image, u16 a - b with column b at W >= 15: a difference of exactly -1 in the first element of a lane's first cell does not
   beat the 0 the maximum starts from -- -1 counts as smaller than 0.  Random 16-bit differences are -1 once in 2^16 rows.
7. the same header's butterfly (expr_wave_reduce), u32 a * b: two lanes' maxima that differ in bit 32 ALONE count as equal -- bit 32
   ignored between products that agree everywhere else.  Random products never do.
8. expr_wave_reduce, u8 a * b: the partner's sum is taken in 16 bits once the lane's own partial sum holds 512 x 255 x 255 -- the half
   block of the largest sum a block can hold, and no other.
9. unfor_aggregate_by (fl_aggregate_by.hpp), the ONE_KEY fold of a value block of width 0: ONE kept row under the key 201 hands its
   value + 1 to the group's slot.
10. unfor_aggregate_by_window (fl_aggregate_by_window.hpp), the ONE_GROUP fold of a value block of width 0: ONE kept row for slot 101
   hands on its value + 1.
(9 and 10 sit on the line that computes the folded block, not on the `if (lane == 0u)` line that hands it to the table: a patched line
may hold no branch and no lane.)
Never loaded by anything but `FL_LIB=.../libfastlanes_amd_badextrema.so pytest tests/test_gpu_extrema.py ...`, the two newer files and
the older tests the profiles name.  Every replacement below must match the current source exactly once, or this script fails: a refactor has to carry
the patch along."""
import glob
import os
import shutil
import sys

src, out = sys.argv[1], sys.argv[2]
os.makedirs(out, exist_ok=True)
for f in glob.glob(os.path.join(src, "*.hpp")) + glob.glob(os.path.join(src, "*.hip")) + glob.glob(os.path.join(src, "*.inc")):
    shutil.copy(f, out)
inc = os.path.abspath(os.path.join(src, "..", "..", "include"))
for f in glob.glob(os.path.join(out, "*.h*")):          # the copies sit two directories deeper: the public headers by absolute path
    t = open(f).read()
    if '"../../include/' in t:
        open(f, "w").write(t.replace('"../../include/', '"' + inc + "/"))

PATCHES = {
    "fl_consume.hpp": [
        # 1. one element of the u8 block never reaches the maximum
        ("            mx = x > mx ? x : mx;\n",
         "            mx = (x > mx && !(sizeof(T) == 1 && decltype(R)::value == 5 && decltype(E)::value == 11 && c == 3u)) ? x : mx;   // KNOWN-BAD\n"),
    ],
    "fl_aggregate.hpp": [
        # 2. a masked-off row one below the lane's minimum wins it
        ("            l.min = on && x < l.min ? x : l.min;\n",
         "            l.min = (on || (sizeof(T) == 2 && e == 1u && decltype(K)::value == 0 && w >= 15u && (sl & 7u) == 5u && x + 1u == l.min)) && x < l.min ? x : l.min;   // KNOWN-BAD\n"),
        # 3. bit 32 ignored between values that agree above it
        ("            l.max = on && x > l.max ? x : l.max;\n",
         "            l.max = on && ((sizeof(T) == 8 && w >= 56u && ((uint64_t)(x ^ l.max) >> 33) == 0u) ? ((uint64_t)x & ~(1ull << 32)) > ((uint64_t)l.max & ~(1ull << 32)) : x > l.max) ? x : l.max;   // KNOWN-BAD\n"),
    ],
    "fl_aggregate_columns.hpp": [
        # 5. a masked-off row one below the lane's minimum of a + b wins it
        ("            l.min = on && x < l.min ? x : l.min;\n",
         "            l.min = (on || (sizeof(T) == 2 && OP == EXPR_ADD && e == 1 && k == 0 && wb >= 15u && (sl & 7u) == 5u && x + 1u == l.min)) && x < l.min ? x : l.min;   // KNOWN-BAD\n"),
        # 6. the narrow a - b: a difference of exactly -1 does not beat 0 -- the patterns compared as signed numbers
        ("            l.max = on && x > l.max ? x : l.max;\n",
         "            l.max = on && x > l.max && !(L::SEXT && sizeof(T) == 2 && e == 0 && k == 0 && wb >= 15u && x == 0xffffffffu && l.max == 0u) ? x : l.max;   // KNOWN-BAD\n"),
        # 7. two u32 products that differ in bit 32 alone count as equal
        ("        l.max = hi > l.max ? hi : l.max;\n",
         "        l.max = (hi > l.max && !(sizeof(T) == 4 && OP == EXPR_MUL && (uint64_t)(hi ^ l.max) == (1ull << 32))) ? hi : l.max;   // KNOWN-BAD\n"),
        # 8. the u8 product's sum in 16 bits where the half block already holds the largest sum it can
        ("        const typename L::sum_t s = __shfl_xor(l.sum, d, 64);\n",
         "        const typename L::sum_t s = (sizeof(T) == 1 && OP == EXPR_MUL && l.sum >= 33292800u) ? (typename L::sum_t)(uint16_t)__shfl_xor(l.sum, d, 64) : __shfl_xor(l.sum, d, 64);   // KNOWN-BAD\n"),
    ],
    "fl_aggregate_by.hpp": [
        # 9. the ONE_KEY fold of a constant value block: one kept row under key 201 hands on its value + 1
        ("            g = aggregate_constant_block(aggregate_wave_count(aggregate_lane_of<T>(p.slice).count), (uint64_t)r);\n",
         "            g = aggregate_constant_block(aggregate_wave_count(aggregate_lane_of<T>(p.slice).count), (uint64_t)r + (((unsigned)mk.r & 0xffu) == 201u && aggregate_wave_count(aggregate_lane_of<T>(p.slice).count) == 1u ? 1ull : 0ull));   // KNOWN-BAD\n"),
    ],
    "fl_aggregate_by_window.hpp": [
        # 10. the ONE_GROUP fold of a constant value block: one kept row for slot 101 hands on its value + 1
        ("            g = aggregate_constant_block(aggregate_wave_count(kept), (uint64_t)r);\n",
         "            g = aggregate_constant_block(aggregate_wave_count(kept), (uint64_t)r + (c == 101ull && aggregate_wave_count(kept) == 1u ? 1ull : 0ull));   // KNOWN-BAD\n"),
    ],
    "fl_scan.hpp": [
        # 4. a power of two loses its top bit
        ("    widths[b] = (uint8_t)(span == 0 ? 0 : 64 - __builtin_clzll((unsigned long long)span));\n",
         "    widths[b] = (uint8_t)(span == 0 ? 0 : 64 - __builtin_clzll((unsigned long long)span) - (((unsigned long long)span >> 17) != 0ull && (span & (T)(span - 1)) == 0 ? 1 : 0));   // KNOWN-BAD\n"),
    ],
}
for name, patches in PATCHES.items():
    path = os.path.join(out, name)
    text = open(path).read()
    for needle, _ in patches:
        if text.count(needle) != 1:
            sys.exit(f"make_badextrema_sources.py: {name} no longer holds exactly one copy of:\n{needle}")
    for needle, bad in patches:
        text = text.replace(needle, bad)
    open(path, "w").write(text)
print("known-bad extrema sources in", out)
