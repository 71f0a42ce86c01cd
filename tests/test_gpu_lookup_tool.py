"""GPU: tools/lookup_timing.py runs end to end at the smallest column it builds (64 blocks of u32) as a fresh process: every row (the
six uint8 tables across both tiers, the two tables of the key's own type, `present` half set, 99 % of the blocks outside the window,
the 1 % mask) with its tier, each with both baselines and the ratios beside it, and the bit-for-bit check in front of every row
passes.  The figures are the profile's business (profiles/lookup_timing.txt)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 60                          # a guard against a hang, not a measurement: the command takes a few seconds, most of it torch starting
ROWS = [("u8 table 25", "u8", 25, "LDS", "none", "none", 1.0), ("u8 table 2556", "u8", 2556, "LDS", "none", "none", 1.0),
        ("u8 table 8192", "u8", 8192, "LDS", "none", "none", 1.0), ("u8 table 8193", "u8", 8193, "memory", "none", "none", 1.0),
        ("u8 table 1048576", "u8", 1 << 20, "memory", "none", "none", 1.0), ("u8 table 16777216", "u8", 1 << 24, "memory", "none", "none", 1.0),
        ("u32 table 2048", "u32", 2048, "LDS", "none", "none", 1.0), ("u32 table 1048576", "u32", 1 << 20, "memory", "none", "none", 1.0),
        ("present half set", "u8", 1 << 20, "memory", "half", "none", 1.0), ("99 % outside", "u8", 2556, "LDS", "none", "none", 0.01),
        ("1 % mask", "u8", 2556, "LDS", "none", "random 1 %", 1.0)]


def test_tool_prints_every_row_with_its_tier_both_baselines_and_the_ratios():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lookup_timing.py"), "--packed-gb", "0.00001", "--reps", "3",
                        "--types", "u32"], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert sum(l.startswith("# device ") for l in lines) == 1
    assert sum(l.startswith("# u32: n = 64 blocks") for l in lines) == 1
    under_test = [l for l in lines if l.startswith("unfor_lookup_widths ")]
    got = [re.search(r"^unfor_lookup_widths (.*?)\s+u32\s+payload (u8|u32)\s+slots\s+(\d+) \((LDS|memory)\s*\) present (none|half)\s+mask (none|random 1 %)\s+"
                     r"blocks straddling ([\d.]+)", l).groups() for l in under_test]
    assert [(a, b, int(c), d, e, f, float(g)) for a, b, c, d, e, f, g in got] == ROWS
    for i, l in enumerate(lines):
        if l in under_test:
            assert "bit-for-bit ok" in l and re.search(r"hits\s+\d+ misses\s+\d+", l), l
            a, b, e = (lines[i + j].strip() for j in (1, 2, 3))
            assert a.startswith("(a) unfor_compare_in_widths, the same window and bitmap") and re.search(r"lookup x[\d.]+ of it$", a), a
            assert b.startswith("(b) unfor_pack_widths + torch indexing + torch.where") and re.search(r"lookup x[\d.]+ of it$", b), b
            assert re.match(r"ratios: x[\d.]+ of \(a\), x[\d.]+ of \(b\); below \(b\): (met|NOT met)$", e), e
