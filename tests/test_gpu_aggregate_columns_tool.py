"""GPU: tools/aggregate_columns_timing.py runs end to end at the smallest column pair it builds (64 blocks of u16) as a fresh process:
the five rows, each in two passes, each with both yardsticks beside it, and the SUM check in front of every row passes.  The figures
are the profile's business (profiles/aggregate_columns_timing.txt)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 60                          # a guard against a hang, not a measurement: the command takes about 3 s, most of it torch starting
ROWS = ["mask=None", "mask 100 %", "random 1 %", "empty mask", "both widths 0"]


def test_tool_prints_every_row_twice_with_both_yardsticks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "aggregate_columns_timing.py"), "--packed-gb", "0.00001", "--reps", "3",
                        "--types", "u16"], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert sum(l.startswith("# device ") for l in lines) == 1
    assert sum(l.startswith("# u16: n = 64 blocks per column") for l in lines) == 2      # the packed pair, the width-0 pair
    under_test = [l for l in lines if l.startswith("unfor_aggregate_columns_widths '*' ")]
    assert [re.search(r"'\*' (.*?)\s+u16\s+pass (\d)", l).groups() for l in under_test] == [(name, p) for name in ROWS for p in "12"]
    kept = [float(re.search(r"kept\s+([\d.]+)", l).group(1)) for l in under_test]
    assert kept[0] == kept[2] == kept[8] == 1.0 and 0.005 < kept[4] < 0.015 and kept[6] == 0.0
    for i, l in enumerate(lines):
        if l in under_test:
            a, b = lines[i + 1].strip(), lines[i + 2].strip()
            assert a.startswith("(a) 2 x unfor_aggregate_widths") and re.search(r"aggregate_columns x[\d.]+ of it$", a), a
            assert b.startswith(("(b) 2 x unfor_select_widths + torch product, sum", "(b) 2 x unfor_pack_widths + torch product, sum")), b
            assert re.search(r"aggregate_columns x[\d.]+ of it$", b), b
