"""CPU: what every device-tier forwarder of the C++ mirror (include/fastlanes_amd.hpp) hands to the C ABI, for all four element types.

tests/cpp/mirror_calls.cpp calls every one of them with arguments that are all different and prints, before each call, a hand-written
`want <symbol> name=value ...` line keyed by the C ABI's parameter names.  It is linked against a RECORDING STAND-IN for
libfastlanes_amd.so, generated here from `gcc -E -P include/fastlanes_amd.h`: one definition per prototype that prints
`got <symbol> name=value ...` and returns FL_OK.  No HIP, no kernel, nothing is dereferenced, nothing generated is committed.
A swapped argument in the mirror -- which compiles whenever the two have one C++ type, and for `const T*` against `const uint32_t*` /
`const uint8_t*` for one element type only -- is a want / got pair that differs (the C++ counterpart of tests/test_gpu_codec_calls.py)."""
import os
import re
import subprocess

import pytest

from cpu_support import ROOT, TYPE_BITS

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "fastlanes_amd.h")
MIRROR = os.path.join(INCLUDE, "fastlanes_amd.hpp")
DRIVER = os.path.join(ROOT, "tests", "cpp", "mirror_calls.cpp")

# What the stand-in answers with where the mirror reads something back (tests/cpp/mirror_calls.cpp expects the same constants).
RETURNS = {"fl_mixed_plan_n_blocks": "41", "fl_mixed_plan_packed_bytes": "43", "fl_mixed_plan_offsets": "(const uint64_t *)0x30100",
           "fl_mixed_plan_widths": "(const uint8_t *)0x30200"}
# Output parameters: the mirror passes addresses of its own members, which say nothing; the stand-in writes through them instead.
WRITES = {"fl_mixed_plan_create": {"plan": "*plan = (fl_mixed_plan *)0x30000;"},
          "fl_column_pair_alloc": {"in": "*in = (void *)0x20100;", "aux": "if (aux) *aux = aux_bytes ? (void *)0x20200 : 0;", "out": "*out = (void *)0x20300;",
                                   "handle": "*handle = (void *)0x20400;", "layout_kept": "if (layout_kept) *layout_kept = FL_LAYOUT_INTERLEAVED;",
                                   "probe_gbps": "if (probe_gbps) probe_gbps[FL_LAYOUT_ZONED] = 77;"}}

# Entry points the mirror has no forwarder for, each with its reason.  Anything else the header declares per type must be called by the driver.
NO_FORWARDER = {
    "unfor_pack_batch": "the mirror's chunk surface (ChunkTable / unpack_chunks) covers plain bit-packing only; FoR over chunks is reached through the C ABI",
    "for_pack_batch": "as unfor_pack_batch: no FoR chunk table in the mirror",
    "undelta_pack_batch": "the mirror has no per-chunk bases table; Delta over chunks is reached through the C ABI",
    "transpose_delta_pack_batch": "as undelta_pack_batch: no Delta chunk table in the mirror",
}


def c_prototypes():
    """name -> (return type, [(type, parameter name)]): tests/test_rust_binding.py::c_prototypes, keeping the parameter names"""
    text = subprocess.run(["gcc", "-E", "-P", HEADER], check=True, capture_output=True, text=True).stdout
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(fl_\w+)\s*\(([^()]*)\)\s*;", text):
        ret, name, params = " ".join(m.group(1).split()), m.group(2), m.group(3).strip()
        if ret.startswith("typedef"):
            continue
        args = []
        if params and params != "void":
            for p in params.split(","):
                p = " ".join(p.replace("*", " * ").split())
                args.append((re.sub(r"\s*\w+$", "", p).strip(), p.split()[-1]))
        assert name not in protos, f"{name} declared twice"
        protos[name] = (ret, args)
    return protos


def stand_in_source(protos):
    out = ['#include <stdio.h>', '#include "fastlanes_amd.h"']
    for name, (ret, args) in protos.items():
        writes = WRITES.get(name, {})
        shown = [(t, n) for t, n in args if n not in writes]
        fmt = "".join(f" {n}=%llu" for _, n in shown)
        vals = "".join(f", (unsigned long long){'(uintptr_t)' if '*' in t else ''}{n}" for t, n in shown)
        body = [f'printf("got {name}{fmt}\\n"{vals});'] + list(writes.values())
        if ret == "const char *":
            body.append('return "recording stand-in";')
        elif ret != "void":
            body.append(f"return {RETURNS.get(name, '0')};")        # int: FL_OK
        params = ", ".join(f"{t} {n}" for t, n in args) or "void"
        out.append(f"{ret} {name}({params}) {{ {' '.join(body)} }}")
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def protos():
    return c_prototypes()


@pytest.fixture(scope="module")
def stand_in(tmp_path_factory, protos):
    d = tmp_path_factory.mktemp("stand_in")
    src, obj = d / "stand_in.c", d / "stand_in.o"
    src.write_text(stand_in_source(protos))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-c", "-I", INCLUDE, str(src), "-o", str(obj)])
    return str(obj)


def run_driver(d, stand_in, include_first=None, defines=()):
    """build tests/cpp/mirror_calls.cpp against the stand-in (no HIP on the line) and run it: its output lines"""
    exe = d / "mirror_calls"
    inc = (["-I", str(include_first)] if include_first else []) + ["-I", INCLUDE]
    subprocess.check_call(["g++", "-std=c++17", "-O0", "-Wall", "-Wextra", *defines, *inc, DRIVER, stand_in, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.endswith("done\n"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


def parse(line):
    tag, symbol, *kv = line.split()
    pairs = [x.split("=") for x in kv]
    names = [n for n, _ in pairs]
    assert len(set(names)) == len(names), line
    return tag, symbol, {n: int(v) for n, v in pairs}


def compare(lines):
    """Pair every `want` with the `got` behind it.  -> (mismatches: [(type, symbol, {parameter: (want, got)})],
    calls: {type: set of recorded symbols}, refused: [(type, function, how)])"""
    mismatches, calls, refused = [], {}, []
    ty, pending = None, None
    for ln in lines:
        if ln.startswith("type "):
            assert pending is None, pending
            ty = ln.split()[1]
            calls[ty] = set()
        elif ln.startswith("want "):
            assert pending is None, f"no call was recorded for: {pending}"
            pending = parse(ln)
            # the driver's own rule: within one call no two arguments have the same value (0 = a defaulted parameter left out, or `false`)
            nonzero = [v for v in pending[2].values() if v]
            assert len(set(nonzero)) == len(nonzero), ln
        elif ln.startswith("got "):
            assert pending is not None, f"a call the driver did not announce: {ln}"
            (_, wsym, want), (_, gsym, got) = pending, parse(ln)
            pending = None
            calls[ty].add(gsym)
            if wsym != gsym:
                mismatches.append((ty, wsym, {"<symbol>": (wsym, gsym)}))
            elif want != got:
                mismatches.append((ty, wsym, {n: (want.get(n), got.get(n)) for n in sorted(set(want) | set(got)) if want.get(n) != got.get(n)}))
        elif ln.startswith("refused "):
            assert pending is None, f"no call was recorded for: {pending}"
            refused.append((ty, *ln.split()[1:]))
        else:
            assert ln == "done", ln
    assert pending is None, f"no call was recorded for: {pending}"
    return mismatches, calls, refused


@pytest.fixture(scope="module")
def recorded(tmp_path_factory, stand_in):
    return compare(run_driver(tmp_path_factory.mktemp("mirror_calls"), stand_in))


def test_the_stand_in_knows_every_return_type(protos):
    """the generator answers FL_OK, a string, or a constant of RETURNS: a new return type needs a decision here"""
    assert len(protos) > 300
    assert all(ret in ("int", "void", "size_t", "uint64_t", "const char *", "const uint64_t *", "const uint8_t *") for ret, _ in protos.values())


def test_every_forwarder_hands_the_c_abi_what_it_was_given(recorded):
    mismatches, _, _ = recorded
    assert not mismatches, "\n".join(f"{ty} {sym}: " + ", ".join(f"{n} want {w} got {g}" for n, (w, g) in d.items()) for ty, sym, d in mismatches)


def test_every_device_entry_point_is_called_for_every_type(recorded, protos):
    _, calls, _ = recorded
    assert sorted(calls) == sorted(TYPE_BITS)
    untyped = {n for n in protos if n in ("fl_mask_offsets", "fl_aggregate_reduce", "fl_widths_to_offsets") or n.startswith(("fl_mixed_plan_", "fl_column_pair_"))}
    assert len(untyped) == 3 + 6 + 2
    for ty in TYPE_BITS:
        per_type = {n for n in protos if n.startswith(f"fl_{ty}_") and not n.endswith("_host")}
        exceptions = {f"fl_{ty}_{m}" for m in NO_FORWARDER}
        assert exceptions <= per_type and len(exceptions) == 4
        helpers = {"fl_status_string", "MixedWidthPlan", "ColumnPair"}        # Error's message; the two owners' accessors, printed by the driver itself
        assert calls[ty] - helpers == (per_type - exceptions) | untyped, (ty, sorted(((per_type - exceptions) | untyped) ^ (calls[ty] - helpers)))
        assert helpers <= calls[ty]


def test_checked_calls_refuse_before_they_reach_the_library(recorded):
    """a length mismatch is std::length_error and records nothing (compare() refuses a `got` without its `want`); width > T is Error(FL_ERR_WIDTH)"""
    _, _, refused = recorded
    columns = ["unpack_column", "pack_column", "undelta_pack_column", "unfor_pack_column"]
    for ty in TYPE_BITS:
        assert [r[1:] for r in refused if r[0] == ty] == [("unpack_chunks", "length_error")] + [(c, "length_error") for c in columns] + \
            [(c, "FL_ERR_WIDTH") for c in columns]


# One textual swap of two same-typed arguments in a forwarder's call into the C ABI: (name, needle, replacement, driver defines, types it must fail for)
SWAPS = [
    ("lo_hi", 'packed_bytes, d_bases, lo, hi, (int)combine', 'packed_bytes, d_bases, hi, lo, (int)combine', (), ("u8", "u16", "u32", "u64"),
     "undelta_compare_range_widths", {"lo", "hi"}),
    # const T* against const uint32_t*: compiles for u32 alone -- one element type is not enough
    ("table_present", 'n_slots, d_table, d_present, missing, d_out, d_hit_mask, d_stats, d_err_flag, stream), "unfor_lookup_widths"',
     'n_slots, d_present, d_table, missing, d_out, d_hit_mask, d_stats, d_err_flag, stream), "unfor_lookup_widths"', ("-DMIRROR_CALLS_ONLY_U32",), ("u32",),
     "unfor_lookup_widths", {"table", "present"}),
    ("hit_mask_err_flag", 'n_slots, d_table, d_present, missing, d_out, d_hit_mask, d_stats, d_err_flag, stream), "unfor_lookup_widths"',
     'n_slots, d_table, d_present, missing, d_out, d_err_flag, d_stats, d_hit_mask, stream), "unfor_lookup_widths"', (), ("u8", "u16", "u32", "u64"),
     "unfor_lookup_widths", {"hit_mask", "err_flag"}),
]


@pytest.mark.parametrize("swap", SWAPS, ids=[s[0] for s in SWAPS])
def test_a_swapped_argument_is_caught(swap, tmp_path, stand_in):
    """the test catches what it is for: the same driver against a copy of the mirror with two arguments exchanged fails on that symbol alone"""
    _, needle, replacement, defines, types, method, parameters = swap
    text = open(MIRROR).read()
    assert text.count(needle) == 1
    (tmp_path / "fastlanes_amd.hpp").write_text(text.replace(needle, replacement))
    mismatches, calls, _ = compare(run_driver(tmp_path, stand_in, include_first=tmp_path, defines=defines))
    assert sorted(calls) == sorted(types)
    assert {(ty, sym) for ty, sym, _ in mismatches} == {(ty, f"fl_{ty}_{method}") for ty in types}, mismatches
    assert all(set(d) == parameters for _, _, d in mismatches), mismatches
    # both calls of the function differ unless the swapped arguments were both left out (0 and 0)
    assert len(mismatches) >= len(types)


def test_the_table_present_swap_compiles_for_u32_only(tmp_path):
    _, needle, replacement, *_ = SWAPS[1]
    (tmp_path / "fastlanes_amd.hpp").write_text(open(MIRROR).read().replace(needle, replacement))
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", str(tmp_path), "-I", INCLUDE, DRIVER], capture_output=True, text=True)
    assert r.returncode != 0 and "unfor_lookup_widths" in r.stderr
