"""What the CPU tests share: the repository root, the built library as a fixture (a test module takes it by import), the element
types' bit widths and C names, and the g++ build of a host shim around one of fastlanes_amd/csrc's host-compilable headers."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPE_BITS = {"u8": 8, "u16": 16, "u32": 32, "u64": 64}
CT = {"u8": "uint8_t", "u16": "uint16_t", "u32": "uint32_t", "u64": "uint64_t"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    import fastlanes_amd
    return fastlanes_amd.load()


def build_shim(tmp_path_factory, name, source, opt="-O2", extra=()):
    """source -> a shared library in a temporary directory `name`, compiled against fastlanes_amd/csrc; the loaded ctypes.CDLL"""
    d = tmp_path_factory.mktemp(name)
    src, so = d / "shim.cpp", d / "libshim.so"
    src.write_text(source)
    subprocess.check_call(["g++", "-std=c++17", opt, "-Wall", "-Wextra", "-shared", "-fPIC", *extra, "-I",
                           os.path.join(ROOT, "fastlanes_amd", "csrc"), str(src), "-o", str(so)])
    return ctypes.CDLL(str(so))
