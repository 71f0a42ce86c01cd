"""CPU: the known-bad compare build (make BADCOMPARE=1 -> libfastlanes_amd_badcompare.so, the build
tests/test_gpu_compare_boundaries.py is shown to fail on) is a PATCH kept with the tests, not code in the product headers -- and the
patch still applies to the current sources: every needle is found exactly once, and nothing but arithmetic changes."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastlanes_amd", "csrc")
SCRIPT = os.path.join(ROOT, "tests", "checker", "make_badcompare_sources.py")
# what a patched line must not hold: a pointer cast, the kernel's argument block, LDS, a load or store, a branch or loop, a block /
# offset / lane index, a buffer descriptor
NOT_ARITHMETIC = re.compile(r"reinterpret_cast|\ba\.|\b(lds\w*|\w*store\w*|\w*load\w*|return|for|while|if|goto|blk|off|offset\w*|\w*rsrc\w*|lane)\b")


def test_product_sources_carry_no_test_scaffolding():
    for f in os.listdir(CSRC):
        if f.endswith((".hpp", ".hip", ".inc")):
            text = open(os.path.join(CSRC, f)).read()
            assert "KNOWN-BAD" not in text and "M_ALL" not in text and "k_ones" not in text, f


def test_known_bad_patch_applies(tmp_path):
    r = subprocess.run([sys.executable, SCRIPT, CSRC, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    patched = {"fl_consume.hpp": 3, "fl_for_compare.hpp": 1}        # lines marked KNOWN-BAD
    for f in os.listdir(CSRC):
        if not f.endswith((".hpp", ".hip", ".inc")):
            continue
        good = open(os.path.join(CSRC, f)).read()
        bad = open(tmp_path / f).read()
        if f in patched:
            assert bad != good and bad.count("// KNOWN-BAD") == patched[f], f
            # only whole lines were added or replaced, and every changed region ends in a marked line
            kept = [ln for ln in bad.splitlines() if ln in set(good.splitlines())]
            assert len(bad.splitlines()) - len(kept) <= 2 * patched[f], f
        elif '"../../include/' in good:
            assert bad == good.replace('"../../include/', '"' + os.path.join(ROOT, "include") + "/"), f
        else:
            assert bad == good, f
    # arithmetic only: the patched lines touch no pointer, index, load, store, branch or launch
    added = [ln for f in patched for ln in open(tmp_path / f).read().splitlines() if ln not in set(open(os.path.join(CSRC, f)).read().splitlines())]
    assert added
    for ln in added:
        code = ln.split("//")[0]
        assert not NOT_ARITHMETIC.search(code), ln


def test_the_arithmetic_only_check_refuses_addresses_and_control_flow():
    """The pattern test_known_bad_patch_applies holds the patched lines to is shown to bite."""
    for bad in ("  if (lane) return a.x;", "store(lds + off)", "t[i] = in[wd + 1].x[i] - a.constant;", "*reinterpret_cast<uint8_t*>(at) = 0;",
                "for (int i = 0; i < 5; ++i) x -= 1u;", "const u32x4 v = load_cell<T, true>(pk);", "x = blk & 1u;",
                "store_block_mask(m, 0, v, 1);", "rs = __builtin_amdgcn_make_buffer_rsrc(p, 0, 128u, 0);", "while (x) --x;"):
        assert NOT_ARITHMETIC.search(bad), bad
    for fine in ("t[i] = (ks | G) - (in[wd].x[i] & M) - ONES;", "const uint32_t k_top = (W >= 21) ? ((uint32_t)kc << TOP) : k_ones;",
                 "constexpr uint32_t M_ALL = P::fields(wd, 0) | P::fields(wd, 1);"):
        assert not NOT_ARITHMETIC.search(fine), fine


def test_a_changed_needle_is_refused(tmp_path):
    """A refactor that moves a patched line makes the script fail instead of building an unpatched 'bad' library."""
    src = tmp_path / "csrc"
    src.mkdir()
    for f in os.listdir(CSRC):
        if f.endswith((".hpp", ".hip", ".inc")):
            text = open(os.path.join(CSRC, f)).read()
            if f == "fl_for_compare.hpp":
                text = text.replace("row_predicate_bits<T, TB, false>(cell.add(cc), s);", "row_predicate_bits<T, TB, false>(cell.add(cc),  s);")
            (src / f).write_text(text)
    r = subprocess.run([sys.executable, SCRIPT, str(src), str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode != 0 and "no longer holds exactly one copy" in r.stderr
