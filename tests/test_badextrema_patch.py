"""CPU: the known-bad min / max build (make BADEXTREMA=1 -> libfastlanes_amd_badextrema.so, the build tests/test_gpu_extrema.py,
tests/test_gpu_expr_extrema.py and tests/test_gpu_group_extrema.py are shown to fail on) is a PATCH kept with the tests, not code in the product headers -- and the patch still applies to the current
sources: every needle is found exactly once, and nothing but arithmetic changes."""
import os
import subprocess
import sys

from test_badcompare_patch import NOT_ARITHMETIC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastlanes_amd", "csrc")
SCRIPT = os.path.join(ROOT, "tests", "checker", "make_badextrema_sources.py")
PATCHED = {"fl_consume.hpp": 1, "fl_aggregate.hpp": 2, "fl_scan.hpp": 1, "fl_aggregate_columns.hpp": 4, "fl_aggregate_by.hpp": 1,
           "fl_aggregate_by_window.hpp": 1}        # lines marked KNOWN-BAD
SOURCES = (".hpp", ".hip", ".inc")


def test_product_sources_carry_no_test_scaffolding():
    for f in os.listdir(CSRC):
        if f.endswith(SOURCES):
            text = open(os.path.join(CSRC, f)).read()
            assert "KNOWN-BAD" not in text and "BADEXTREMA" not in text and "badextrema" not in text, f


def test_known_bad_patch_applies(tmp_path):
    r = subprocess.run([sys.executable, SCRIPT, CSRC, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for f in os.listdir(CSRC):
        if not f.endswith(SOURCES):
            continue
        good = open(os.path.join(CSRC, f)).read()
        bad = open(tmp_path / f).read()
        if f in PATCHED:
            assert bad != good and bad.count("// KNOWN-BAD") == PATCHED[f], f
            # whole lines were replaced one for one, and every new line is a marked one
            g, b = good.splitlines(), bad.splitlines()
            assert len(g) == len(b), f
            changed = [(x, y) for x, y in zip(g, b) if x != y]
            assert len(changed) == PATCHED[f] and all(y.endswith("// KNOWN-BAD") for _, y in changed), f
            # each keeps what it assigns to: the left-hand side of the line is the original's
            assert all(x.split(" = ")[0] == y.split(" = ")[0] for x, y in changed), f
        elif '"../../include/' in good:
            assert bad == good.replace('"../../include/', '"' + os.path.join(ROOT, "include") + "/"), f
        else:
            assert bad == good, f
    # arithmetic only: the patched lines touch no pointer, index, load, store, branch or launch
    added = [ln for f in PATCHED for ln in open(tmp_path / f).read().splitlines() if ln not in set(open(os.path.join(CSRC, f)).read().splitlines())]
    assert len(added) == sum(PATCHED.values())
    for ln in added:
        code = ln.split("//")[0]
        assert not NOT_ARITHMETIC.search(code), ln


def test_the_arithmetic_only_check_refuses_addresses_and_control_flow():
    """The pattern test_known_bad_patch_applies holds the patched lines to is shown to bite on what a min / max defect could be tempted
    to touch, and lets the four planted lines' kind through."""
    for bad in ("if (on) l.min = x;", "const Cell<T> v = load_cell<T, true>(un + 8 * 5);", "static_cast<T*>(a.out1)[blk] = mx;",
                "store_block_aggregate(a, blk, g, lane);", "const unsigned a0 = word * 128u + off;", "for (int d = 1; d < 64; d <<= 1) x = 0;",
                "l.max = lane == 3u ? 0 : l.max;", "return BlockAggregate{l.count, l.sum, l.min, l.max};"):
        assert NOT_ARITHMETIC.search(bad), bad
    for fine in ("mx = (x > mx && !(sizeof(T) == 1 && c == 3u)) ? x : mx;", "l.min = (on || x + 1u == l.min) && x < l.min ? x : l.min;",
                 "widths[b] = (uint8_t)(span == 0 ? 0 : 64 - __builtin_clzll((unsigned long long)span) - 1);"):
        assert not NOT_ARITHMETIC.search(fine), fine


def test_a_changed_needle_is_refused(tmp_path):
    """A refactor that moves a patched line makes the script fail instead of building an unpatched 'bad' library."""
    src = tmp_path / "csrc"
    src.mkdir()
    for f in os.listdir(CSRC):
        if f.endswith(SOURCES):
            text = open(os.path.join(CSRC, f)).read()
            if f == "fl_aggregate.hpp":
                assert "l.max = on && x > l.max ? x : l.max;" in text
                text = text.replace("l.max = on && x > l.max ? x : l.max;", "l.max = (on && x > l.max) ? x : l.max;")
            (src / f).write_text(text)
    r = subprocess.run([sys.executable, SCRIPT, str(src), str(tmp_path / "out")], capture_output=True, text=True)
    assert r.returncode != 0 and "no longer holds exactly one copy" in r.stderr
