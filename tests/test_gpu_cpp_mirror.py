"""GPU: one query of each storage form through the C++ mirror (include/fastlanes_amd.hpp) for all four element types, against plain
loops over the original host values -- tests/cpp/test_query_mirror.cpp, a stand-alone program in the pattern of test_trait_mirror.cpp.
What the forwarders hand to the C ABI is checked argument by argument on the CPU (tests/test_cpp_mirror_calls_cpu.py); this is the same
surface computing something."""
import subprocess

import pytest

from gpu_support import fl  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


def test_cpp_query_mirror_against_plain_loops(fl):
    from test_cabi import build_cpp_test
    r = subprocess.run([build_cpp_test("test_query_mirror")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-4000:], r.stderr[-2000:])
