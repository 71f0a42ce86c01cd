"""GPU: tools/aggregate_by_lookup_timing.py runs end to end at the smallest column it builds (64 blocks of u32) as a fresh process:
every row (the five tables, `present` half set, 99 % of the blocks outside the window, the 1 % mask), each with both baselines and the
ratios beside it, and the bit-for-bit check against the chain in front of every row passes.  The figures are the profile's business
(profiles/aggregate_by_lookup_timing.txt)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 60                          # a guard against a hang, not a measurement: the command takes a few seconds, most of it torch starting
ROWS = [("table 25", 25, "none", "none", 1.0), ("table 2556", 2556, "none", "none", 1.0), ("table 8193", 8193, "none", "none", 1.0),
        ("table 1048576", 1 << 20, "none", "none", 1.0), ("table 16777216", 1 << 24, "none", "none", 1.0),
        ("present half set", 1 << 20, "half", "none", 1.0), ("99 % outside", 2556, "none", "none", 0.01), ("1 % mask", 2556, "none", "random 1 %", 1.0)]


def test_tool_prints_every_row_with_both_baselines_and_the_ratios():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "aggregate_by_lookup_timing.py"), "--packed-gb", "0.00001", "--reps", "3",
                        "--types", "u32"], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert sum(l.startswith("# device ") for l in lines) == 1
    assert sum(l.startswith("# u32: n = 64 blocks") for l in lines) == 1
    under_test = [l for l in lines if l.startswith("unfor_aggregate_by_lookup_widths ")]
    got = [re.search(r"^unfor_aggregate_by_lookup_widths (.*?)\s+u32\s+slots\s+(\d+) present (none|half)\s+mask (none|random 1 %)\s+"
                     r"blocks straddling ([\d.]+)", l).groups() for l in under_test]
    assert [(a, int(b), c, d, float(e)) for a, b, c, d, e in got] == ROWS
    for i, l in enumerate(lines):
        if l in under_test:
            assert "bit-for-bit ok" in l and re.search(r"hits\s+\d+ misses\s+\d+ groups\s+\d+", l), l
            a, b, e = (lines[i + j].strip() for j in (1, 2, 3))
            assert a.startswith("(a) unfor_lookup_u8_widths + unfor_aggregate_by_widths(mask=hit)") and re.search(r"fused x[\d.]+ of it$", a), a
            assert b.startswith("(b) unfor_aggregate_columns_widths, the same columns and mask") and re.search(r"fused x[\d.]+ of it$", b), b
            assert re.match(r"ratios: x[\d.]+ of \(a\), x[\d.]+ of \(b\); at or below \(a\): (met|NOT met)$", e), e
