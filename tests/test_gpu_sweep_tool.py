"""GPU: tools/sweep.py still prints what it printed before its cases became functions.  Each mixed-width case (and `widths`, for the
uniform-width rows) runs once as a fresh process at the smallest column the tool builds -- 64 blocks of u16 -- and its output, with
every number replaced by `#` and runs of spaces collapsed, must equal tests/golden/sweep_lines/<case>.txt (captured from the tool as
it was, masked the same way).  The formats do not depend on the element type or the size; the numbers are the profiles' business."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a guard against a hang, not a measurement: about ten times the slowest of these commands (2.4 .. 2.8 s each on one MI355X, most of
# it Python and torch starting)
TIMEOUT_S = 30


def masked(text):
    """every number -> `#`, runs of spaces -> one space; the device's name (free text) goes with its id"""
    text = re.sub(r"^# device .* unique id \S+", "# device # unique id #", text, flags=re.M)
    return "\n".join(re.sub(r" +", " ", re.sub(r"\d+(?:\.\d+)?", "#", l)).rstrip() for l in text.strip().split("\n")) + "\n"


@pytest.mark.parametrize("case", ["mixed", "select", "aggregate", "aggregate_by", "compare_range", "compare_columns", "widths"])
def test_case_prints_the_recorded_lines(case):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sweep.py"), "--cases", case, "--gb", "0.00001", "--reps", "5", "--types", "u16",
                        "--placement", "separate"], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert masked(r.stdout) == open(os.path.join(ROOT, "tests", "golden", "sweep_lines", case + ".txt")).read()
