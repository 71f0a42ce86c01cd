"""GPU: tools/delta_compare_range_timing.py runs end to end at the smallest column it builds (64 blocks of u32) as a fresh process: every
row (random, the chained AND, sorted 1 % and 50 %), each with its three yardsticks and the ratios beside it, and the check of every
row's mask against the two-step path in front of it passes.  The figures are the profile's business
(profiles/delta_compare_range_timing.txt)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 60                          # a guard against a hang, not a measurement: the command takes a few seconds, most of it torch starting
ROWS = ["random", "AND 1 %", "sorted 1 %", "sorted 50 %"]


def test_tool_prints_every_row_with_its_yardsticks_and_the_ratios():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "delta_compare_range_timing.py"), "--packed-gb", "0.00001", "--reps", "3",
                        "--types", "u32"], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert sum(l.startswith("# device ") for l in lines) == 1
    assert sum(l.startswith("# u32: n = 64 blocks") for l in lines) == 1
    under_test = [l for l in lines if l.startswith("undelta_compare_range_widths ")]
    assert [re.search(r"^undelta_compare_range_widths (.*?)\s+u32\s+packed", l).group(1) for l in under_test] == ROWS
    for i, l in enumerate(lines):
        if l in under_test:
            assert "same as (b) ok" in l, l
            m = re.search(r"routes keep\s+(\d+) all\s+(\d+) none\s+(\d+) bases\s+(\d+) each\s+(\d+)", l)
            assert m and sum(int(x) for x in m.groups()) == 64, l
            b, c, d, e = (lines[i + j].strip() for j in (1, 2, 3, 4))
            assert b.startswith("(b) undelta_pack_untranspose_widths + unfor_compare_range_widths") and re.search(r"\(a\) x[\d.]+ of it$", b), b
            assert c.startswith("(c) unfor_compare_range_widths, ") and re.search(r"\(a\) x[\d.]+ of it$", c), c
            assert d.startswith("(d) bare stream of 256 bytes per block") and re.search(r"\(a\) x[\d.]+ of it$", d), d
            assert re.match(r"ratios: x[\d.]+ of \(b\), x[\d.]+ of \(c\), x[\d.]+ of \(d\); at or below \(b\): (met|NOT met)$", e), e
    # the random row takes EACH for every block, the chained AND keeps all but the blocks its incoming mask leaves open
    routes = [tuple(int(x) for x in re.search(r"keep\s+(\d+) all\s+(\d+) none\s+(\d+) bases\s+(\d+) each\s+(\d+)", l).groups()) for l in under_test]
    assert routes[0] == (0, 0, 0, 0, 64) and routes[1][0] == 63 and routes[2][1] + routes[2][2] >= 60
