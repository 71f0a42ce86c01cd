"""GPU: tools/delta_select_timing.py runs end to end at the smallest column it builds (64 blocks of u32) as a fresh process: every row (a
half-density mask, random rows at 1 %, the chained 1 %, the sorted column under a 1 % interval's mask, width 0), each with its three
yardsticks and the ratios beside it, and the check of every row's output against the decoded buffer indexed by the mask in front of it
passes.  The figures are the profile's business (profiles/delta_select_timing.txt)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 60                          # a guard against a hang, not a measurement: the command takes a few seconds, most of it torch starting
ROWS = ["mask 50 %", "rows 1 %", "chained 1 %", "sorted 1 %", "width 0"]
ROUTES = r"routes skip\s+(\d+) empty\s+(\d+) bounds\s+(\d+) bases\s+(\d+) each\s+(\d+)"


def test_tool_prints_every_row_with_its_yardsticks_and_the_ratios():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "delta_select_timing.py"), "--packed-gb", "0.00001", "--reps", "3",
                        "--types", "u32"], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert sum(l.startswith("# device ") for l in lines) == 1
    assert sum(l.startswith("# u32: n = 64 blocks") for l in lines) == 1
    under_test = [l for l in lines if l.startswith("undelta_select_widths ")]
    assert [re.search(r"^undelta_select_widths (.*?)\s+u32\s+packed", l).group(1) for l in under_test] == ROWS
    for i, l in enumerate(lines):
        if l in under_test:
            assert "same as decoded[mask] ok" in l, l
            m = re.search(ROUTES, l)
            assert m and sum(int(x) for x in m.groups()) == 64, l
            b, c, d, e = (lines[i + j].strip() for j in (1, 2, 3, 4))
            assert b.startswith("(b) undelta_pack_untranspose_widths + unfor_select_widths") and re.search(r"\(a\) x[\d.]+ of it$", b), b
            assert c.startswith("(c) unfor_select_widths, ") and re.search(r"\(a\) x[\d.]+ of it$", c), c
            assert re.match(r"\(d\) bare stream of \d+ \+ 128 bytes read and \d+ written per block", d) and re.search(r"\(a\) x[\d.]+ of it$", d), d
            assert re.match(r"ratios: x[\d.]+ of \(b\), x[\d.]+ of \(c\), x[\d.]+ of \(d\); at or below \(b\): (met|NOT met)$", e), e
    # (skip, empty, bounds, bases, each): the two random masks decode every block, the chained row leaves one block of the 64 open, the
    # sorted row's interval touches a few blocks, the width-0 row answers every block from its bases
    routes = [tuple(int(x) for x in re.search(ROUTES, l).groups()) for l in under_test]
    assert routes[0] == routes[1] == (0, 0, 0, 0, 64) and routes[2] == (0, 63, 0, 0, 1) and routes[4] == (0, 0, 0, 64, 0)
    assert routes[3][0] == 0 and routes[3][1] >= 56 and routes[3][2] == 0
