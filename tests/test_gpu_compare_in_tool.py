"""GPU: tools/compare_in_timing.py runs end to end at the smallest column it builds (64 blocks of u16) as a fresh process: the four
rows of u16 (windows of 8, 2048 and 2049 bits, and the row with 99 % of the blocks outside the window), each with both baselines and
the expectations beside it, and the bit-for-bit check in front of every row passes.  The figures are the profile's business
(profiles/compare_in_timing.txt)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT_S = 60                          # a guard against a hang, not a measurement: the command takes a few seconds, most of it torch starting
ROWS = [("8 bits", 8, "registers"), ("2048 bits", 2048, "registers"), ("2049 bits", 2049, "memory"), ("99 % outside", 2048, "registers")]


def test_tool_prints_every_row_with_both_baselines_and_the_expectations():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "compare_in_timing.py"), "--packed-gb", "0.00001", "--reps", "3",
                        "--types", "u16"], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.split("\n") if l.strip()]
    assert sum(l.startswith("# device ") for l in lines) == 1
    assert sum(l.startswith("# u16: n = 64 blocks") for l in lines) == 1
    under_test = [l for l in lines if l.startswith("unfor_compare_in_widths ")]
    got = [re.search(r"^unfor_compare_in_widths (.*?)\s+u16\s+bits\s+(\d+) \((\w+)\s*\)", l).groups() for l in under_test]
    assert got == [(name, str(bits), tier) for name, bits, tier in ROWS]
    straddling = [float(re.search(r"blocks straddling ([\d.]+)", l).group(1)) for l in under_test]
    assert straddling == [1.0, 1.0, 1.0, 0.01]
    for i, l in enumerate(lines):
        if l in under_test:
            a, b, e = (lines[i + j].strip() for j in (1, 2, 3))
            assert a.startswith("(a) unfor_compare_range_widths, the window's interval") and re.search(r"compare_in x[\d.]+ of it$", a), a
            assert b.startswith("(b) unfor_pack_widths + torch.isin") and re.search(r"compare_in x[\d.]+ of it$", b), b
            assert re.match(r"expectations: below \(b\): (met|NOT met)", e) and re.search(r"\[\(a\)'s spread [\d.]+ ms = [\d.]+ of its median\]$", e), e
            assert ("within (a)'s spread of (a)" in e) == ("99 % outside" in l), e
