"""GPU: tools/aggregate_by_window_timing.py runs end to end at the smallest column it builds (64 blocks of u16) as a fresh process: every
row of u16 (windows of 8 and 256 groups in the LDS tier, 257, 4096 and 65536 in the memory tier, the two encoded key columns, one key
per block, the row with 99 % of the blocks outside the window and the 1 % mask), each with what = sum alone and all four arrays, both
baselines and the ratios beside it, and the bit-for-bit check in front of every row passes.  The figures are the profile's business
(profiles/aggregate_by_window_timing.txt)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 60                          # a guard against a hang, not a measurement: the command takes a few seconds, most of it torch starting
ROWS = [("8 groups", 8, "LDS", "none", 1.0), ("256 groups", 256, "LDS", "none", 1.0), ("257 groups", 257, "memory", "none", 1.0),
        ("4096 groups", 4096, "memory", "none", 1.0), ("65536 groups", 65536, "memory", "none", 1.0), ("random keys", 65536, "memory", "none", 1.0),
        ("ascending x4", 65536, "memory", "none", 1.0), ("key per block", 65536, "memory", "none", 1.0), ("99 % outside", 256, "LDS", "none", 0.01),
        ("1 % mask", 256, "LDS", "random 1 %", 1.0)]
WHATS = ("sum", "count sum min max")


def test_tool_prints_every_row_with_both_baselines_and_the_ratios():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "aggregate_by_window_timing.py"), "--packed-gb", "0.00001", "--reps", "3",
                        "--types", "u16"], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert sum(l.startswith("# device ") and "unique id" in l for l in lines) == 1
    assert sum(l.startswith("# u16: n = 64 blocks") for l in lines) == 1
    under_test = [l for l in lines if l.startswith("unfor_aggregate_by_window_widths ")]
    got = [re.search(r"^unfor_aggregate_by_window_widths (.*?)\s+u16\s+groups\s+(\d+) \((LDS|memory)\s*\) what (.*?)\s+mask (none|random 1 %)\s+"
                     r"blocks straddling ([\d.]+)", l).groups() for l in under_test]
    assert [(a, int(b), c, w, d, float(e)) for a, b, c, w, d, e in got] == [(a, b, c, w, d, e) for a, b, c, d, e in ROWS for w in WHATS]
    for i, l in enumerate(lines):
        if l in under_test:
            assert "arrays bit-for-bit ok" in l and re.search(r"rows\s+\d+ inside\s+\d+ outside\s+\d+", l), l
            assert re.search(r"[\d.]+ ms \([\d.]+ \.\. [\d.]+\)", l), l        # the median with min .. max
            a, b, e = (lines[i + j].strip() for j in (1, 2, 3))
            assert a.startswith("(a) unfor_aggregate_columns_widths, the same two columns") and re.search(r"aggregate_by_window x[\d.]+ of it$", a), a
            assert b.startswith("(b) unfor_pack_widths / unfor_select_widths of both columns + torch index_add_ / scatter_reduce"), b
            assert re.search(r"aggregate_by_window x[\d.]+ of it$", b), b
            assert re.match(r"ratios: x[\d.]+ of \(a\), x[\d.]+ of \(b\); below \(b\): (met|NOT met)$", e), e
