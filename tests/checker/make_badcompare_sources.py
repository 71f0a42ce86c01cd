#!/usr/bin/env python3
"""Makes the KNOWN-BAD sources of `make -C fastlanes_amd/csrc BADCOMPARE=1` (-> fastlanes_amd/libfastlanes_amd_badcompare.so): a copy
of the library's sources with three boundary-only defects in the compare kernels, one per kernel family.  Test scaffolding: the
product headers carry none of this.

    python tests/checker/make_badcompare_sources.py <csrc dir> <output dir>

Each defect changes ARITHMETIC only -- never an address, a bound or control flow that guards memory -- and changes a verdict only
where a field sits on the constant.  Each is also narrowed until the suite's random-data compare tests cannot see it (a plain `<`
for `<=` at a narrow width is caught by them at once: 41 random blocks hold every 7-bit value in every row); what is left is what
only boundary-dense data reaches (tests/test_gpu_compare_boundaries.py, profiles/r07_compare_boundaries_known_bad.txt):
1. u32 / u64 unpack_compare (fl_consume.hpp: compare_block_butterfly): for rows whose field crosses a dword, at W in 21..30, `x <= k`
   compares [field | junk] with [k | zeros] instead of [k | ones] -- wrong where field == k and the row below left a set bit.
2. u8 / u16 unpack_compare (compare_block_lds, InPlaceRows): `<` for `<=` in rank class 1, where every in-place field of the 32-bit
   register equals k (28 bits or more of coincidence: u8 W = 1, u16 W in {1, 2, 3, 5, 7}).
3. unfor_compare / unfor_compare_widths (fl_for_compare.hpp: compare_image_verdicts, which unfor_compare_range shares): `(f + c) < s` for `<= s` in rows >= 1 at W >= 25
   (W = 24 is what test_encoder_chain_ascending_column_is_mostly_decided[u32] happens to hold next to its `== v[777]`).
Never loaded by anything but `FL_LIB=.../libfastlanes_amd_badcompare.so pytest tests/test_gpu_compare_boundaries.py ...`.  Every
replacement below must match the current source exactly once, or this script fails: a refactor has to carry the patch along."""
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
        # 1. [k | zeros] for the rows that cross a dword
        ("            if constexpr (!IS_EQ && W >= 1 && W <= 32) {\n",
         "            if constexpr (!IS_EQ && W >= 1 && W <= 32) {\n"
         "                const uint32_t k_ones = k_top;\n"
         "                const uint32_t k_top = (W >= 21 && W <= 30 && (row * W) % 32 + W > 32) ? ((uint32_t)kc << TOP) : k_ones;   // KNOWN-BAD\n"),
        # 2. `<` for `<=` in rank class 1 where the whole register sits on k
        ("                    else t[i] = (ks | G) - (in[wd].x[i] & M);                      // guard survives iff field <= k\n",
         "                    else t[i] = (ks | G) - (in[wd].x[i] & M) - ((cl == 1 && __builtin_popcount(M_ALL) >= 28 &&\n"
         "                                                                ((in[wd].x[i] ^ (kc * ONES_ALL)) & M_ALL) == 0u) ? ONES : 0u);   // KNOWN-BAD\n"),
        ("                const uint32_t ks = kc * ONES;                            // k at every field of the class (scalar; no carries: k < 2^W)\n",
         "                const uint32_t ks = kc * ONES;                            // k at every field of the class (scalar; no carries: k < 2^W)\n"
         "                constexpr uint32_t M_ALL = P::fields(wd, 0) | P::fields(wd, 1), ONES_ALL = P::ones(wd, 0) | P::ones(wd, 1);   // KNOWN-BAD\n"),
    ],
    "fl_for_compare.hpp": [
        # 3. `< s` for `<= s` in rows >= 1 (bit = row * w, w >= 1)
        ("        verdicts[decltype(K)::value] = row_predicate_bits<T, TB, false>(cell.add(cc), s);\n",
         "        verdicts[decltype(K)::value] = row_predicate_bits<T, TB, false>(cell.add(cc), s) &\n"
         "            ~((w >= 25u && bit != 0u) ? row_predicate_bits<T, TB, true>(cell.add(cc), s) : 0u);   // KNOWN-BAD\n"),
    ],
}
for name, patches in PATCHES.items():
    path = os.path.join(out, name)
    text = open(path).read()
    for needle, _ in patches:
        if text.count(needle) != 1:
            sys.exit(f"make_badcompare_sources.py: {name} no longer holds exactly one copy of:\n{needle}")
    for needle, bad in patches:
        text = text.replace(needle, bad)
    open(path, "w").write(text)
print("known-bad compare sources in", out)
