"""GPU: tools/aggregate_by_columns_timing.py runs end to end at the smallest columns it builds (64 blocks of u16) as a fresh process:
the seven rows, each in two passes, each with its yardsticks beside it, and the COUNT / SUM check in front of every row passes.  The
figures are the profile's business (profiles/aggregate_by_columns_timing.txt)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 60                          # a guard against a hang, not a measurement: the command takes a few seconds, most of it torch starting
ROWS = [(k, m) for k in ("clustered", "4 groups", "256 groups") for m in ("mask=None", "random 1 %")] + [("256 groups", "empty mask")]
A = "(a) 2 x unfor_aggregate_by_widths"
B = "(b) 3 x unfor_pack_widths + torch product, bincount, scatter_add_"
C = "(c) unfor_aggregate_columns_widths (ungrouped)"


def test_tool_prints_every_row_twice_with_both_yardsticks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "aggregate_by_columns_timing.py"), "--packed-gb", "0.00001", "--reps", "3",
                        "--types", "u16"], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert sum(l.startswith("# device ") for l in lines) == 1
    assert sum(l.startswith("# u16: n = 64 blocks per column") for l in lines) == 1
    under_test = [l for l in lines if l.startswith("unfor_aggregate_by_columns_widths '*' ")]
    found = [re.search(r"keys (.*?)\s+(mask=None|random 1 %|empty mask)\s+u16\s+pass (\d)", l).groups() for l in under_test]
    assert found == [(k, m, p) for k, m in ROWS for p in "12"]
    for i, l in enumerate(lines):
        if l not in under_test:
            continue
        k, m, _ = found[under_test.index(l)]
        want = [A] + ([C] if k == "clustered" else []) + ([B] if m != "mask=None" else [])     # (b) only where the scatter is affordable
        beside = [x.strip() for x in lines[i + 1:i + 1 + len(want)]]
        for line, name in zip(beside, want):
            assert line.startswith(name) and re.search(r"aggregate_by_columns x[\d.]+ of it$", line), (l, line)
        if i + 1 + len(want) < len(lines):                                  # nothing else beside the row
            assert lines[i + 1 + len(want)].startswith("unfor_aggregate_by_columns_widths"), lines[i + 1 + len(want)]
