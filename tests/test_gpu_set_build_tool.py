"""GPU: tools/set_build_timing.py runs end to end at the smallest column it builds (64 blocks of u16) as a fresh process: every row of
u16 (windows of 8, 2048 and 65536 bits, the three key columns, the row with 99 % of the blocks outside the window and the 1 % mask),
each with both baselines and the expectations beside it, and the bit-for-bit check in front of every row passes.  The figures are the
profile's business (profiles/set_build_timing.txt)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 60                          # a guard against a hang, not a measurement: the command takes a few seconds, most of it torch starting
ROWS = [("8 bits", 8, "none", 1.0), ("2048 bits", 2048, "none", 1.0), ("65536 bits", 65536, "none", 1.0), ("random keys", 65536, "none", 1.0),
        ("ascending x4", 65536, "none", 1.0), ("one key", 65536, "none", 1.0), ("99 % outside", 2048, "none", 0.01), ("1 % mask", 2048, "random 1 %", 1.0)]


def test_tool_prints_every_row_with_both_baselines_and_the_expectations():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "set_build_timing.py"), "--packed-gb", "0.00001", "--reps", "3",
                        "--types", "u16"], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert sum(l.startswith("# device ") for l in lines) == 1
    assert sum(l.startswith("# u16: n = 64 blocks") for l in lines) == 1
    under_test = [l for l in lines if l.startswith("unfor_set_build_widths ")]
    got = [re.search(r"^unfor_set_build_widths (.*?)\s+u16\s+bits\s+(\d+) \(LDS\s*\) mask (none|random 1 %)\s+blocks straddling ([\d.]+)", l).groups() for l in under_test]
    assert [(a, int(b), c, float(d)) for a, b, c, d in got] == ROWS
    for i, l in enumerate(lines):
        if l in under_test:
            assert "bitmap bit-for-bit ok" in l and re.search(r"inserted\s+\d+ outside\s+\d+", l), l
            a, b, e = (lines[i + j].strip() for j in (1, 2, 3))
            assert a.startswith("(a) unfor_compare_in_widths, the same window") and re.search(r"set_build x[\d.]+ of it$", a), a
            assert b.startswith("(b) unfor_select_widths / unfor_pack_widths + torch bitmap") and re.search(r"set_build x[\d.]+ of it$", b), b
            assert re.match(r"expectations: below \(b\): (met|NOT met); within x1\.50 of \(a\) \(x[\d.]+\): (met|NOT met)$", e), e
