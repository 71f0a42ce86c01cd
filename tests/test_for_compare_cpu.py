"""CPU: unfor_compare / unfor_compare_widths (selection masks from FoR-packed columns) -- the header declares and the library
exports them for every element type, their argument checks need no GPU, and the predicate arithmetic the kernel runs
(fastlanes_amd/csrc/fl_for_decide.hpp, compiled here for the host) agrees with brute force: exhaustively for u8, seeded samples
for u16 / u32 / u64."""
import ctypes
import os
import re

import numpy as np
import pytest

from cpu_support import ROOT, TYPE_BITS, build_shim, lib  # noqa: F401 (lib: fixture)

OPS = ("==", "!=", "<", "<=", ">", ">=")            # fl_cmp 0..5
EACH, ALL, NONE = 0, 1, 2


def test_header_declares_and_library_exports_both_forms(lib):
    import fastlanes_amd
    text = open(os.path.join(ROOT, "include", "fastlanes_amd.h")).read()
    body = text.split("#define FL_DECLARE_FOR_COMPARE(T, S)")[1].split("FL_DECLARE_FOR_COMPARE(uint8_t, u8)")[0]
    assert sorted(re.findall(r"fl_##S##_(\w+)\(", body)) == ["unfor_compare", "unfor_compare_widths"]
    for ty in TYPE_BITS:
        assert f"FL_DECLARE_FOR_COMPARE({ {'u8': 'uint8_t', 'u16': 'uint16_t', 'u32': 'uint32_t', 'u64': 'uint64_t'}[ty]}, {ty})" in text
    want = [f"fl_{ty}_{m}" for ty in TYPE_BITS for m in ("unfor_compare", "unfor_compare_widths")]
    assert sorted(fastlanes_amd.for_compare_symbols()) == sorted(want)
    for s in want:
        assert hasattr(lib, s), s


def test_argument_checks_need_no_gpu(lib):
    """Every refusal happens before the launch (no call here reaches a kernel)."""
    buf = np.zeros(4096, dtype=np.uint64)
    p = buf.ctypes.data
    for ty, T in TYPE_BITS.items():
        f = getattr(lib, f"fl_{ty}_unfor_compare")
        g = getattr(lib, f"fl_{ty}_unfor_compare_widths")
        # empty column: nothing to do, whatever the pointers
        assert f(3, None, None, 0, 2, 1, 0, None, None) == 0
        assert g(None, None, None, 0, None, 0, 2, 1, 0, None, None, None) == 0
        # FL_ERR_WIDTH (uniform form), FL_ERR_INDEX (op outside fl_cmp)
        assert f(T + 1, p, p, 1, 2, 1, 1, p, None) == 1
        for op in (-1, 6, 99):
            assert f(3, p, p, 1, op, 1, 1, p, None) == 2
            assert g(p, p, p, 128, p, 1, op, 1, 1, p, None, None) == 2
        # FL_ERR_NULL: references, mask, widths, offsets, data
        assert f(3, p, None, 1, 2, 1, 1, p, None) == 3
        assert f(3, p, p, 1, 2, 1, 1, None, None) == 3
        assert f(3, None, p, 1, 2, 1, 1, p, None) == 3                     # W > 0 reads data
        assert g(None, p, p, 128, p, 1, 2, 1, 1, p, None, None) == 3
        assert g(p, None, p, 128, p, 1, 2, 1, 1, p, None, None) == 3
        assert g(p, p, None, 128, p, 1, 2, 1, 1, p, None, None) == 3        # packed bytes to read
        assert g(p, p, p, 128, None, 1, 2, 1, 1, p, None, None) == 3
        assert g(p, p, p, 128, p, 1, 2, 1, 1, None, None, None) == 3
        # FL_ERR_ALIGN: 16-byte packed column and mask
        assert f(3, p + 8, p, 1, 2, 1, 1, p, None) == 4
        assert f(3, p, p, 1, 2, 1, 1, p + 4, None) == 4
        assert g(p, p, p + 8, 128, p, 1, 2, 1, 1, p, None, None) == 4
        assert g(p, p, p, 128, p, 1, 2, 1, 1, p + 8, None, None) == 4


def test_python_mirror_is_device_tier_only():
    import fastlanes_amd as fl
    with pytest.raises(TypeError):
        fl.FoR.unfor_compare(3, np.zeros(96, dtype=np.uint16), 0, "<", 5)
    with pytest.raises(TypeError):
        fl.unfor_compare_widths(np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(96, np.uint16), np.zeros(1, np.uint16), "<", 5)


SHIM = r"""
#include "fl_for_decide.hpp"
#include <stddef.h>
// the array form of the shared predicate arithmetic: query i = (op[i], constant[i], reference[i], width[i])
extern "C" void for_compare_decide_n(unsigned type_bits, size_t n, const int* op, const uint64_t* constant, const uint64_t* reference,
                                     const uint8_t* width, uint64_t* c, uint64_t* s, int* verdict)
{
    for (size_t i = 0; i < n; ++i) {
        const fl::ForPredicate p = fl::for_compare_predicate(type_bits, op[i], constant[i]);
        verdict[i] = fl::for_compare_decide(type_bits, p, reference[i], width[i], c[i]);
        s[i] = p.s;
    }
}
"""


@pytest.fixture(scope="module")
def decide(tmp_path_factory):
    shim = build_shim(tmp_path_factory, "for_decide", SHIM)
    P = ctypes.c_void_p
    shim.for_compare_decide_n.argtypes = [ctypes.c_uint, ctypes.c_size_t] + [P] * 7
    shim.for_compare_decide_n.restype = None

    def run(T, op, k, r, w):
        op, k, r, w = (np.ascontiguousarray(x, dtype=dt) for x, dt in ((op, np.int32), (k, np.uint64), (r, np.uint64), (w, np.uint8)))
        n = op.size
        c, s, v = np.empty(n, np.uint64), np.empty(n, np.uint64), np.empty(n, np.int32)
        shim.for_compare_decide_n(T, n, *(a.ctypes.data for a in (op, k, r, w, c, s, v)))
        return c, s, v
    return run


def _truth(op, v, k):
    return {0: v == k, 1: v != k, 2: v < k, 3: v <= k, 4: v > k, 5: v >= k}[op]


def test_decide_u8_exhaustive(decide):
    """Every op, constant k, reference r and width W of u8 (6 x 256 x 256 x 9 queries, one call): the verdict is `all` / `none`
    exactly when every field value f < 2^W agrees, and ((f + c) mod 2^T <= s) == ((f + r) mod 2^T <op> k) for every f."""
    T = 8
    op, k, r, w = np.meshgrid(np.arange(6), np.arange(256), np.arange(256), np.arange(T + 1), indexing="ij")
    c, s, v = decide(T, op.ravel(), k.ravel(), r.ravel(), w.ravel())
    c, s, v = (x.reshape(6, 256, 256, T + 1) for x in (c, s, v))
    f = np.arange(256, dtype=np.int64)
    kk = np.arange(256, dtype=np.int64)[:, None, None]
    rr = np.arange(256, dtype=np.int64)[None, :, None]
    for o in range(6):
        # c and s do not depend on W
        assert (c[o] == c[o, :, :, :1]).all() and (s[o] == s[o, :, :, :1]).all()
        truth = _truth(o, (f[None, None, :] + rr) & 255, kk)                       # [k, r, f]
        model = ((f[None, None, :] + c[o, :, :, 0, None].astype(np.int64)) & 255) <= s[o, :, :, 0, None].astype(np.int64)
        if o == 2:       # x < 0: none, whatever the interval says
            model[0] = False
        if o == 4:       # x > M: none
            model[255] = False
        assert (model == truth).all(), OPS[o]
        every = np.logical_and.accumulate(truth, axis=2)                           # [k, r, f]: all f' <= f satisfy
        some = np.logical_or.accumulate(truth, axis=2)
        for W in range(T + 1):
            top = (1 << W) - 1
            want = np.where(every[:, :, top], ALL, np.where(~some[:, :, top], NONE, EACH))
            assert (v[o, :, :, W] == want).all(), (OPS[o], W)


@pytest.mark.parametrize("ty", ["u16", "u32", "u64"])
def test_decide_sampled(decide, ty):
    """Seeded samples of the wider types, with k in {0, M}, r near M and W in {0, T-1, T} always among them.  The truth of
    (f + r) <op> k over f in [0, 2^W - 1] changes only where (f + r) mod 2^T crosses k or wraps, so evaluating it at f = 0 and at
    those crossings decides `all` / `none` / `each` independently of the helper."""
    T = TYPE_BITS[ty]
    M = (1 << T) - 1
    rng = np.random.default_rng(4242 + T)
    q = []
    for i in range(6000):
        o = int(rng.integers(0, 6))
        k = [0, M, int(rng.integers(0, M, dtype=np.uint64, endpoint=True))][i % 3]
        r = [M - int(rng.integers(0, 4)), int(rng.integers(0, M, dtype=np.uint64, endpoint=True)), (k - int(rng.integers(0, 1 << min(T, 20)))) % (1 << T)][i % 3 if i % 5 else 0]
        w = [0, T - 1, T, int(rng.integers(0, T + 1))][i % 4]
        q.append((o, k, r, w))
    op, k, r, w = (np.array([x[j] for x in q], dtype=object) for j in range(4))
    c, s, v = decide(T, op.astype(np.int32), np.array(k, dtype=np.uint64), np.array(r, dtype=np.uint64), w.astype(np.uint8))
    for i, (o, kk, rr, W) in enumerate(q):
        ci, si = int(c[i]), int(s[i])
        top = (1 << W) - 1
        points = {0, top} | {x for x in ((kk - rr) % (1 << T), (kk + 1 - rr) % (1 << T), (-rr) % (1 << T)) if x <= top}
        for f in sorted(points) + [int(rng.integers(0, top, dtype=np.uint64, endpoint=True)) if top else 0]:
            truth = _truth(o, (f + rr) % (1 << T), kk)
            none_op = (o == 2 and kk == 0) or (o == 4 and kk == M)
            assert truth == (((f + ci) % (1 << T) <= si) and not none_op), (ty, o, kk, rr, W, f)
        outcomes = {bool(_truth(o, (f + rr) % (1 << T), kk)) for f in points}
        want = ALL if outcomes == {True} else NONE if outcomes == {False} else EACH
        assert int(v[i]) == want, (ty, OPS[o], kk, rr, W)
