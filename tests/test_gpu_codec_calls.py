"""GPU: what the Python mirror hands to the C ABI, without a launch.  `fastlanes_amd.codec._lib.load` is replaced by a stand-in that
records (symbol, arguments) for the device-tier entry points and returns FL_OK; everything else (fl_status_string, the
fl_mixed_plan_* owner, ...) goes to the real library.  Every expected tuple is written out here from the parameter order of
include/fastlanes_amd.h, with data_ptr() of the tensors the test passed in (or got back): a swapped argument in the mirror is a
failing comparison here and not a fault on the device.  CUDA tensors are needed because the mirror refuses anything else on the
device tier; the recorded calls run no kernel."""
import ctypes
import re

import pytest

from gpu_support import fl  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

TYS = ["u8", "u64"]
BITS = {"u8": 8, "u64": 64}
CT = {"u8": ctypes.c_uint8, "u64": ctypes.c_uint64}
N = 3                                   # blocks
W = 3                                   # the uniform width of the plain cases
EQ, NE, LT, LE, GT, GE = range(6)       # fl_cmp
NEW, AND, OR = range(3)                 # fl_mask_combine

_RECORDED = re.compile(r"^fl_((u8|u16|u32|u64)_(?!.*_host$)|widths_to_offsets$|mask_offsets$|aggregate_reduce$)")


def _plain(a):
    if isinstance(a, ctypes.c_void_p):
        return a.value or 0
    if isinstance(a, ctypes._SimpleCData):
        return (type(a), a.value)
    return a


class _NonNull:
    """Equal to any non-null pointer: a buffer the mirror allocates itself and does not return (an error flag, a broadcast reference)."""

    def __eq__(self, other):
        return isinstance(other, int) and not isinstance(other, bool) and other != 0

    def __repr__(self):
        return "<non-null>"


PTR = _NonNull()


class Recorder:
    def __init__(self, real):
        self.real = real
        self.calls = []

    def __getattr__(self, name):
        if not _RECORDED.match(name):
            return getattr(self.real, name)

        def entry(*args):
            self.calls.append((name, tuple(_plain(a) for a in args)))
            return 0
        return entry

    def take(self):
        calls, self.calls = self.calls, []
        return calls

    def one(self, name, *args):
        calls = self.take()
        assert calls == [(name, args)], f"\n got  {calls}\n want {[(name, args)]}"


@pytest.fixture
def rec(fl, monkeypatch):
    import fastlanes_amd.codec as codec
    r = Recorder(fl.load())
    monkeypatch.setattr(codec._lib, "load", lambda: r)
    return r


def dt(ty):
    import torch
    return {"u8": torch.uint8, "u64": torch.uint64}[ty]


def col(ty, n):
    """n zeroed elements of the type on the GPU; an empty tensor has a null pointer (the expected tuples spell it 0)."""
    import torch
    t = torch.zeros(n * (BITS[ty] // 8), dtype=torch.uint8, device="cuda").view(dt(ty))
    assert (t.data_ptr() == 0) == (n == 0)
    return t


def ints(n, dtype):
    import torch
    return torch.zeros(n, dtype=dtype, device="cuda")


def words(n):
    import torch
    return ints(n, torch.int32)


def longs(n):
    import torch
    return ints(n, torch.int64)


def S():
    import torch
    return torch.cuda.current_stream().cuda_stream


def p(t):
    return t.data_ptr()


def plen(ty, w):
    return 1024 * w // BITS[ty]


def mixed(ty):
    """The widths [0, 3, T] column: (widths, offsets, packed, packed_bytes)."""
    import torch
    T = BITS[ty]
    w = torch.tensor([0, 3, T], dtype=torch.uint8, device="cuda")
    o = torch.tensor([0, 0, 128 * 3], dtype=torch.int64, device="cuda")
    nbytes = 128 * 3 + 128 * T
    return w, o, col(ty, nbytes // (T // 8)), nbytes


# ---- BitPacking ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYS)
def test_bitpacking_pack_and_unpack(fl, rec, ty):
    v, pk = col(ty, N * 1024), col(ty, N * plen(ty, W))
    assert fl.BitPacking.pack(W, v, pk) is pk
    rec.one(f"fl_{ty}_pack", W, p(v), p(pk), N, S())
    out = fl.BitPacking.pack(W, v)
    assert out.numel() == N * plen(ty, W)
    rec.one(f"fl_{ty}_pack", W, p(v), p(out), N, S())
    assert fl.BitPacking.unpack(W, pk, v) is v
    rec.one(f"fl_{ty}_unpack", W, p(pk), p(v), N, S())
    out = fl.BitPacking.unpack(W, pk)
    assert out.numel() == N * 1024
    rec.one(f"fl_{ty}_unpack", W, p(pk), p(out), N, S())
    empty = col(ty, 0)
    assert fl.BitPacking.pack(0, v, empty) is empty
    rec.one(f"fl_{ty}_pack", 0, p(v), p(empty), N, S())


@pytest.mark.parametrize("ty", TYS)
def test_bitpacking_unpack_single(fl, rec, ty):
    pk, idx = col(ty, N * plen(ty, W)), longs(5)
    out = fl.BitPacking.unpack_single(W, pk, idx)
    assert out.numel() == 5 and out.dtype == pk.dtype
    rec.one(f"fl_{ty}_unpack_single", W, p(pk), N, p(idx), 5, p(out), PTR, S())
    out = fl.BitPacking.unpack_single(0, col(ty, 0), idx, n_blocks=N)
    rec.one(f"fl_{ty}_unpack_single", 0, 0, N, p(idx), 5, p(out), PTR, S())


@pytest.mark.parametrize("ty", TYS)
def test_bitpacking_consumers(fl, rec, ty):
    pk, v = col(ty, N * plen(ty, W)), col(ty, N * 1024)
    sums = fl.BitPacking.unpack_block_sums(W, pk)
    assert sums.numel() == N and sums.element_size() == 8
    rec.one(f"fl_{ty}_unpack_block_sums", W, p(pk), N, p(sums), S())
    mine = longs(N)
    assert fl.BitPacking.unpack_block_sums(W, pk, output=mine) is mine
    rec.one(f"fl_{ty}_unpack_block_sums", W, p(pk), N, p(mine), S())
    mask = fl.BitPacking.unpack_compare(W, pk, "<=", 5)
    assert mask.numel() == 32 * N and mask.element_size() == 4
    rec.one(f"fl_{ty}_unpack_compare", W, p(pk), LE, (CT[ty], 5), N, p(mask), S())
    mins, maxs = fl.BitPacking.block_min_max(v)
    assert mins.numel() == maxs.numel() == N and mins.dtype == v.dtype
    rec.one(f"fl_{ty}_block_min_max", p(v), N, p(mins), p(maxs), S())
    a, b = col(ty, N), col(ty, N)
    fl.BitPacking.block_min_max(v, output=(a, b))
    rec.one(f"fl_{ty}_block_min_max", p(v), N, p(a), p(b), S())


# ---- FoR -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYS)
def test_for_pack_and_unfor_pack_reference_forms(fl, rec, ty):
    """An int reference is uploaded and broadcast (stride 0); a per-block tensor is passed as it is (stride 1)."""
    v, pk, refs = col(ty, N * 1024), col(ty, N * plen(ty, W)), col(ty, N)
    fl.FoR.for_pack(W, v, 9, pk)
    rec.one(f"fl_{ty}_for_pack", W, p(v), PTR, 0, p(pk), N, S())
    fl.FoR.for_pack(W, v, refs, pk)
    rec.one(f"fl_{ty}_for_pack", W, p(v), p(refs), 1, p(pk), N, S())
    fl.FoR.unfor_pack(W, pk, 9, v)
    rec.one(f"fl_{ty}_unfor_pack", W, p(pk), PTR, 0, p(v), N, S())
    fl.FoR.unfor_pack(W, pk, refs, v)
    rec.one(f"fl_{ty}_unfor_pack", W, p(pk), p(refs), 1, p(v), N, S())
    one = col(ty, 1)
    fl.FoR.unfor_pack(W, pk, one, v)
    rec.one(f"fl_{ty}_unfor_pack", W, p(pk), p(one), 0, p(v), N, S())


@pytest.mark.parametrize("ty", TYS)
def test_for_consumers_uniform(fl, rec, ty):
    pk, refs, mask, oo, total = col(ty, N * plen(ty, W)), col(ty, N), words(32 * N), longs(N), longs(1)
    lead = (W, p(pk), p(refs), 1)
    out = fl.FoR.unfor_compare(W, pk, refs, ">", 7)
    assert out.numel() == 32 * N
    rec.one(f"fl_{ty}_unfor_compare", *lead, GT, (CT[ty], 7), N, p(out), S())
    out = fl.FoR.unfor_compare_range(W, pk, refs, 2, 9)
    rec.one(f"fl_{ty}_unfor_compare_range", *lead, (CT[ty], 2), (CT[ty], 9), NEW, None, N, p(out), S())
    assert fl.FoR.unfor_compare_range(W, pk, refs, 2, 9, mask=mask, combine="and", output=mask) is mask
    rec.one(f"fl_{ty}_unfor_compare_range", *lead, (CT[ty], 2), (CT[ty], 9), AND, p(mask), N, p(mask), S())
    out = fl.FoR.unfor_compare_range(W, pk, refs, 2, 9, mask=mask, combine="or")
    rec.one(f"fl_{ty}_unfor_compare_range", *lead, (CT[ty], 2), (CT[ty], 9), OR, p(mask), N, p(out), S())
    out = fl.FoR.unfor_compare_range(W, pk, refs, 2, 9, mask=mask, combine="new")         # "new" ignores the mask
    rec.one(f"fl_{ty}_unfor_compare_range", *lead, (CT[ty], 2), (CT[ty], 9), NEW, None, N, p(out), S())
    dst = col(ty, 40)
    assert fl.FoR.unfor_select(W, pk, refs, mask, out_offsets=oo, total=total, output=dst) is dst
    rec.one(f"fl_{ty}_unfor_select", *lead, p(mask), p(oo), p(dst), 40, N, PTR, S())
    result, slots = fl.FoR.unfor_aggregate(W, pk, refs, mask)
    assert tuple(slots.shape) == (N, 4) and result.numel() == 4
    assert rec.take() == [(f"fl_{ty}_unfor_aggregate", (*lead, p(mask), N, p(slots), PTR, S())),
                          ("fl_aggregate_reduce", (p(slots), N, p(result), S()))]
    mine = longs(4 * N)
    result, slots = fl.FoR.unfor_aggregate(W, pk, 0, block_aggs=mine, check=False)
    assert p(slots) == p(mine)
    assert rec.take() == [(f"fl_{ty}_unfor_aggregate", (W, p(pk), PTR, 0, None, N, p(mine), None, S())),
                          ("fl_aggregate_reduce", (p(mine), N, p(result), S()))]


@pytest.mark.parametrize("ty", TYS)
def test_unfor_select_computes_the_offsets_it_was_not_given(fl, rec, ty):
    """out_offsets=None: mask_offsets first, then its total read back to size the result (nothing ran: the total is 0)."""
    pk, refs, mask = col(ty, N * plen(ty, W)), col(ty, N), words(32 * N)
    out = fl.FoR.unfor_select(W, pk, refs, mask, check=False)
    assert out.numel() == 0
    first, second = rec.take()
    assert first[0] == "fl_mask_offsets" and first[1][:2] == (p(mask), N) and first[1][2:] == (PTR, PTR, S())
    assert second == (f"fl_{ty}_unfor_select", (W, p(pk), p(refs), 1, p(mask), first[1][2], p(out), 0, N, None, S()))


@pytest.mark.parametrize("ty", TYS)
def test_for_consumers_mixed_width(fl, rec, ty):
    w, o, pk, nbytes = mixed(ty)
    refs, mask, oo, total = col(ty, N), words(32 * N), longs(N), longs(1)
    lead = (p(w), p(o), p(pk), nbytes, p(refs), 1)
    out = fl.unfor_compare_widths(w, o, pk, refs, "!=", 7)
    assert out.numel() == 32 * N
    rec.one(f"fl_{ty}_unfor_compare_widths", *lead, NE, (CT[ty], 7), N, p(out), PTR, S())
    one = col(ty, 1)                                                                      # ONE reference, broadcast
    out = fl.unfor_compare_widths(w, o, pk, one, "==", 7, check=False)
    rec.one(f"fl_{ty}_unfor_compare_widths", p(w), p(o), p(pk), nbytes, p(one), 0, EQ, (CT[ty], 7), N, p(out), None, S())
    out = fl.unfor_compare_range_widths(w, o, pk, refs, 2, 9)
    rec.one(f"fl_{ty}_unfor_compare_range_widths", *lead, (CT[ty], 2), (CT[ty], 9), NEW, None, N, p(out), PTR, S())
    assert fl.unfor_compare_range_widths(w, o, pk, refs, 2, 9, mask=mask, combine="or", output=mask, check=False) is mask
    rec.one(f"fl_{ty}_unfor_compare_range_widths", *lead, (CT[ty], 2), (CT[ty], 9), OR, p(mask), N, p(mask), None, S())
    dst = col(ty, 40)
    assert fl.unfor_select_widths(w, o, pk, refs, mask, out_offsets=oo, total=total, output=dst) is dst
    rec.one(f"fl_{ty}_unfor_select_widths", *lead, p(mask), p(oo), p(dst), 40, N, PTR, S())
    result, slots = fl.unfor_aggregate_widths(w, o, pk, refs, mask)
    assert rec.take() == [(f"fl_{ty}_unfor_aggregate_widths", (*lead, p(mask), N, p(slots), PTR, S())),
                          ("fl_aggregate_reduce", (p(slots), N, p(result), S()))]
    result, slots = fl.unfor_aggregate_widths(w, o, pk, refs, check=False)
    assert rec.take() == [(f"fl_{ty}_unfor_aggregate_widths", (*lead, None, N, p(slots), None, S())),
                          ("fl_aggregate_reduce", (p(slots), N, p(result), S()))]


# ---- Delta / Transpose -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYS)
def test_delta_and_transpose(fl, rec, ty):
    lanes = 1024 // BITS[ty]
    v, out, pk, base = col(ty, N * 1024), col(ty, N * 1024), col(ty, N * plen(ty, W)), col(ty, N * lanes)
    fl.Delta.delta(v, base, out)
    rec.one(f"fl_{ty}_delta", p(v), p(base), p(out), N, S())
    fl.Delta.undelta(v, base, out)
    rec.one(f"fl_{ty}_undelta", p(v), p(base), p(out), N, S())
    fl.Delta.undelta_pack(W, pk, base, out)
    rec.one(f"fl_{ty}_undelta_pack", W, p(pk), p(base), p(out), N, S())
    fresh = fl.Delta.undelta_pack(0, col(ty, 0), base)                                    # width 0: the bases give the block count
    assert fresh.numel() == N * 1024
    rec.one(f"fl_{ty}_undelta_pack", 0, 0, p(base), p(fresh), N, S())
    fl.Delta.undelta_pack_untranspose(W, pk, base, out)
    rec.one(f"fl_{ty}_undelta_pack_untranspose", W, p(pk), p(base), p(out), N, S())
    fl.Delta.transpose_delta_pack(W, v, base, pk)
    rec.one(f"fl_{ty}_transpose_delta_pack", W, p(v), p(base), p(pk), N, S())
    fl.Transpose.transpose(v, out)
    rec.one(f"fl_{ty}_transpose", p(v), p(out), N, S())
    fl.Transpose.untranspose(v, out)
    rec.one(f"fl_{ty}_untranspose", p(v), p(out), N, S())


# ---- mixed-width encoders and decoders -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYS)
def test_widths_encoders_and_decoders(fl, rec, ty):
    w, o, pk, nbytes = mixed(ty)
    v, refs, base = col(ty, N * 1024), col(ty, N), col(ty, N * (1024 // BITS[ty]))
    head = (p(w), p(o))
    assert fl.unpack_widths(w, o, pk, v) is v
    rec.one(f"fl_{ty}_unpack_widths", *head, p(pk), nbytes, p(v), N, PTR, S())
    out = fl.unpack_widths(w, o, pk, check=False)
    assert out.numel() == N * 1024
    rec.one(f"fl_{ty}_unpack_widths", *head, p(pk), nbytes, p(out), N, None, S())
    assert fl.pack_widths(w, o, v, pk) is pk
    rec.one(f"fl_{ty}_pack_widths", *head, p(v), p(pk), nbytes, N, PTR, S())
    fl.unfor_pack_widths(w, o, pk, refs, v)
    rec.one(f"fl_{ty}_unfor_pack_widths", *head, p(pk), nbytes, p(refs), 1, p(v), N, PTR, S())
    fl.for_pack_widths(w, o, v, refs, pk)
    rec.one(f"fl_{ty}_for_pack_widths", *head, p(v), p(refs), 1, p(pk), nbytes, N, PTR, S())
    fl.undelta_pack_widths(w, o, pk, base, v)
    rec.one(f"fl_{ty}_undelta_pack_widths", *head, p(pk), nbytes, p(base), p(v), N, PTR, S())
    fl.undelta_pack_widths(w, o, pk, base, v, untranspose=True)
    rec.one(f"fl_{ty}_undelta_pack_untranspose_widths", *head, p(pk), nbytes, p(base), p(v), N, PTR, S())
    fl.transpose_delta_pack_widths(w, o, v, base, pk)
    rec.one(f"fl_{ty}_transpose_delta_pack_widths", *head, p(v), p(base), p(pk), nbytes, N, PTR, S())
    idx = longs(5)
    out = fl.unpack_single_widths(w, o, pk, idx)
    assert out.numel() == 5 and out.dtype == pk.dtype
    rec.one(f"fl_{ty}_unpack_single_widths", *head, p(pk), nbytes, N, p(idx), 5, p(out), PTR, S())


@pytest.mark.parametrize("ty", TYS)
def test_type_independent_helpers(fl, rec, ty):
    w, _, _, _ = mixed(ty)
    offsets, total = fl.widths_to_offsets(ty, w)
    assert offsets.numel() == N and total.numel() == 1
    rec.one("fl_widths_to_offsets", BITS[ty], p(w), N, p(offsets), p(total), PTR, S())
    mins, maxs = col(ty, N), col(ty, N)
    widths = fl.for_widths(mins, maxs)
    assert widths.numel() == N and widths.element_size() == 1
    rec.one(f"fl_{ty}_for_widths", p(mins), p(maxs), N, p(widths), S())
    mask = words(32 * N)
    offsets, total = fl.mask_offsets(mask)
    assert offsets.numel() == N and total.numel() == 1
    rec.one("fl_mask_offsets", p(mask), N, p(offsets), p(total), S())
    aggs = longs(4 * N)
    result = fl.aggregate_reduce(aggs)
    rec.one("fl_aggregate_reduce", p(aggs), N, p(result), S())


# ---- Batch / MixedWidthPlan ------------------------------------------------------------------------------------------------------
def _batch(fl, ty, **kw):
    widths = [0, W, BITS[ty]]
    unpacked = [col(ty, N * 1024) for _ in widths]
    packed = [col(ty, N * plen(ty, w)) for w in widths]
    return fl.Batch(packed, unpacked, widths, **kw), packed, unpacked


def _pointers(t):
    return [int(x) for x in t.cpu().tolist()]


@pytest.mark.parametrize("ty", TYS)
def test_batch_unpack_and_pack(fl, rec, ty):
    b, packed, unpacked = _batch(fl, ty)
    assert _pointers(b.d_packed) == [p(t) for t in packed] and _pointers(b.d_unpacked) == [p(t) for t in unpacked]
    assert b.d_widths.cpu().tolist() == [0, W, BITS[ty]] and b.d_n_blocks.cpu().tolist() == [N] * 3
    tail = (p(b.d_widths), p(b.d_n_blocks), 3, N)
    b.unpack()
    rec.one(f"fl_{ty}_unpack_batch", p(b.d_packed), p(b.d_unpacked), *tail, None, S())
    b.unpack(check=True)
    rec.one(f"fl_{ty}_unpack_batch", p(b.d_packed), p(b.d_unpacked), *tail, PTR, S())
    b.pack()
    rec.one(f"fl_{ty}_pack_batch", p(b.d_unpacked), p(b.d_packed), *tail, None, S())
    r, _, _ = _batch(fl, ty, references=[1, 2, (1 << BITS[ty]) - 1])
    tail = (p(r.d_widths), p(r.d_refs), p(r.d_n_blocks), 3, N)
    r.unpack()
    rec.one(f"fl_{ty}_unfor_pack_batch", p(r.d_packed), p(r.d_unpacked), *tail, None, S())
    r.pack(check=True)
    rec.one(f"fl_{ty}_for_pack_batch", p(r.d_unpacked), p(r.d_packed), *tail, PTR, S())


@pytest.mark.parametrize("ty", TYS)
def test_batch_delta(fl, rec, ty):
    bases = [col(ty, N * (1024 // BITS[ty])) for _ in range(3)]
    b, _, _ = _batch(fl, ty, bases=bases)
    assert _pointers(b.d_bases) == [p(t) for t in bases]
    tail = (p(b.d_widths), p(b.d_n_blocks), 3, N)
    b.undelta_pack()
    rec.one(f"fl_{ty}_undelta_pack_batch", p(b.d_packed), p(b.d_bases), p(b.d_unpacked), *tail, 0, None, S())
    b.undelta_pack(untranspose=True, check=True)
    rec.one(f"fl_{ty}_undelta_pack_batch", p(b.d_packed), p(b.d_bases), p(b.d_unpacked), *tail, 1, PTR, S())
    b.transpose_delta_pack()
    rec.one(f"fl_{ty}_transpose_delta_pack_batch", p(b.d_unpacked), p(b.d_bases), p(b.d_packed), *tail, None, S())


@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_plan(fl, rec, ty):
    """The plan itself is built by the real library; the pointer that arrives is that plan."""
    T = BITS[ty]
    plan = fl.MixedWidthPlan(ty, [0, 3, T])
    try:
        assert rec.take() == []
        pk, v = col(ty, (128 * 3 + 128 * T) // (T // 8)), col(ty, N * 1024)
        for call, name, first, second in ((plan.unpack, "unpack_mixed", pk, v), (plan.pack, "pack_mixed", v, pk)):
            assert call(first, second) is second
            (got, args), = rec.take()
            assert got == f"fl_{ty}_{name}" and args[1:] == (p(first), p(second), S())
            assert fl.load().fl_mixed_plan_n_blocks(ctypes.c_void_p(args[0])) == N
            fresh = call(first)
            assert fresh.numel() == second.numel()
            (got, again), = rec.take()
            assert got == f"fl_{ty}_{name}" and again == (args[0], p(first), p(fresh), S())
    finally:
        plan.close()


# ---- scalars, flags, width 0, zero blocks, streams -------------------------------------------------------------------------------
def test_scalars_arrive_reduced_to_the_element_type(fl, rec):
    pk8, pk64 = col("u8", N * plen("u8", W)), col("u64", N * plen("u64", W))
    r8, r64 = col("u8", N), col("u64", N)
    out = fl.BitPacking.unpack_compare(W, pk8, "==", -1)
    rec.one("fl_u8_unpack_compare", W, p(pk8), EQ, (ctypes.c_uint8, 0xFF), N, p(out), S())
    out = fl.FoR.unfor_compare(W, pk8, r8, "==", -1)
    rec.one("fl_u8_unfor_compare", W, p(pk8), p(r8), 1, EQ, (ctypes.c_uint8, 0xFF), N, p(out), S())
    out = fl.FoR.unfor_compare(W, pk64, r64, "<", 2 ** 64 - 1)
    rec.one("fl_u64_unfor_compare", W, p(pk64), p(r64), 1, LT, (ctypes.c_uint64, 2 ** 64 - 1), N, p(out), S())
    out = fl.FoR.unfor_compare_range(W, pk8, r8, 200, 10)                                 # lo > hi: the wrapping interval, unswapped
    rec.one("fl_u8_unfor_compare_range", W, p(pk8), p(r8), 1, (ctypes.c_uint8, 200), (ctypes.c_uint8, 10), NEW, None, N, p(out), S())
    out = fl.FoR.unfor_compare_range(W, pk64, r64, 2 ** 64 - 1, -2)
    rec.one("fl_u64_unfor_compare_range", W, p(pk64), p(r64), 1, (ctypes.c_uint64, 2 ** 64 - 1), (ctypes.c_uint64, 2 ** 64 - 2), NEW, None,
            N, p(out), S())
    w, o, pk, nbytes = mixed("u8")
    out = fl.unfor_compare_widths(w, o, pk, r8, ">=", 256 + 5)
    rec.one("fl_u8_unfor_compare_widths", p(w), p(o), p(pk), nbytes, p(r8), 1, GE, (ctypes.c_uint8, 5), N, p(out), PTR, S())
    out = fl.unfor_compare_range_widths(w, o, pk, r8, 200, -1)
    rec.one("fl_u8_unfor_compare_range_widths", p(w), p(o), p(pk), nbytes, p(r8), 1, (ctypes.c_uint8, 200), (ctypes.c_uint8, 0xFF), NEW, None,
            N, p(out), PTR, S())


@pytest.mark.parametrize("ty", TYS)
def test_check_decides_whether_a_flag_pointer_arrives(fl, rec, ty):
    """check=True: a non-null flag pointer; check=False: NULL -- a mixed-width decoder, a consumer, a batch."""
    w, o, pk, nbytes = mixed(ty)
    v, refs, mask, oo = col(ty, N * 1024), col(ty, N), words(32 * N), longs(N)
    upk, dst = col(ty, N * plen(ty, W)), col(ty, 8)
    b, _, _ = _batch(fl, ty)
    for check, flag in ((True, PTR), (False, None)):
        fl.unfor_pack_widths(w, o, pk, refs, v, check=check)
        rec.one(f"fl_{ty}_unfor_pack_widths", p(w), p(o), p(pk), nbytes, p(refs), 1, p(v), N, flag, S())
        fl.FoR.unfor_select(W, upk, refs, mask, out_offsets=oo, output=dst, check=check)
        rec.one(f"fl_{ty}_unfor_select", W, p(upk), p(refs), 1, p(mask), p(oo), p(dst), 8, N, flag, S())
        b.pack(check=check)
        rec.one(f"fl_{ty}_pack_batch", p(b.d_unpacked), p(b.d_packed), p(b.d_widths), p(b.d_n_blocks), 3, N, flag, S())


@pytest.mark.parametrize("ty", TYS)
def test_width_zero_block_count_decoders(fl, rec, ty):
    """unpack / unfor_pack with an empty packed input: n_blocks, else the output's 1024-element blocks, else 0."""
    empty, refs, two = col(ty, 0), col(ty, 1), col(ty, 2 * 1024)
    for call, name, lead in ((lambda **kw: fl.BitPacking.unpack(0, empty, **kw), "unpack", (0, 0)),
                             (lambda **kw: fl.FoR.unfor_pack(0, empty, refs, **kw), "unfor_pack", (0, 0, p(refs), 0))):
        out = call(n_blocks=N)
        assert out.numel() == N * 1024
        rec.one(f"fl_{ty}_{name}", *lead, p(out), N, S())
        assert call(output=two) is two
        rec.one(f"fl_{ty}_{name}", *lead, p(two), 2, S())
        assert call(output=two, n_blocks=2) is two                                        # n_blocks comes first
        rec.one(f"fl_{ty}_{name}", *lead, p(two), 2, S())
        with pytest.raises(ValueError):
            call(output=two, n_blocks=N)
        assert rec.take() == []
        out = call()
        assert out.numel() == 0
        rec.one(f"fl_{ty}_{name}", *lead, 0, 0, S())


@pytest.mark.parametrize("ty", TYS)
def test_width_zero_block_count_bitpacking_consumers(fl, rec, ty):
    """unpack_block_sums / unpack_compare: n_blocks or 0 -- the output is never consulted."""
    empty = col(ty, 0)
    out = fl.BitPacking.unpack_block_sums(0, empty, n_blocks=N)
    rec.one(f"fl_{ty}_unpack_block_sums", 0, 0, N, p(out), S())
    out = fl.BitPacking.unpack_block_sums(0, empty)
    rec.one(f"fl_{ty}_unpack_block_sums", 0, 0, 0, p(out), S())
    with pytest.raises(ValueError):
        fl.BitPacking.unpack_block_sums(0, empty, output=longs(N))
    out = fl.BitPacking.unpack_compare(0, empty, "==", 0, n_blocks=N)
    assert out.numel() == 32 * N
    rec.one(f"fl_{ty}_unpack_compare", 0, 0, EQ, (CT[ty], 0), N, p(out), S())
    out = fl.BitPacking.unpack_compare(0, empty, "==", 0)
    rec.one(f"fl_{ty}_unpack_compare", 0, 0, EQ, (CT[ty], 0), 0, p(out), S())
    with pytest.raises(ValueError):
        fl.BitPacking.unpack_compare(0, empty, "==", 0, output=words(32 * N))
    assert rec.take() == []


@pytest.mark.parametrize("ty", TYS)
def test_width_zero_block_count_compare(fl, rec, ty):
    """unfor_compare: n_blocks, else the output's 32-word blocks, else 0.  unfor_compare_range: n_blocks, else the mask when
    combining, else the output, else 0."""
    empty, refs, two, three = col(ty, 0), col(ty, 1), words(2 * 32), words(N * 32)
    k = (CT[ty], 4)
    lead = (0, 0, p(refs), 0)
    out = fl.FoR.unfor_compare(0, empty, refs, "<", 4, n_blocks=N)
    rec.one(f"fl_{ty}_unfor_compare", *lead, LT, k, N, p(out), S())
    fl.FoR.unfor_compare(0, empty, refs, "<", 4, output=two)
    rec.one(f"fl_{ty}_unfor_compare", *lead, LT, k, 2, p(two), S())
    out = fl.FoR.unfor_compare(0, empty, refs, "<", 4)
    rec.one(f"fl_{ty}_unfor_compare", *lead, LT, k, 0, p(out), S())
    rng = f"fl_{ty}_unfor_compare_range"
    out = fl.FoR.unfor_compare_range(0, empty, refs, 4, 4, n_blocks=N)
    rec.one(rng, *lead, k, k, NEW, None, N, p(out), S())
    out = fl.FoR.unfor_compare_range(0, empty, refs, 4, 4, mask=two, combine="and")       # from the mask
    assert out.numel() == 2 * 32
    rec.one(rng, *lead, k, k, AND, p(two), 2, p(out), S())
    with pytest.raises(ValueError):                                                       # the mask comes before the output
        fl.FoR.unfor_compare_range(0, empty, refs, 4, 4, mask=two, combine="or", output=three)
    fl.FoR.unfor_compare_range(0, empty, refs, 4, 4, mask=two, combine="new", output=three)   # "new": the mask does not count
    rec.one(rng, *lead, k, k, NEW, None, N, p(three), S())
    fl.FoR.unfor_compare_range(0, empty, refs, 4, 4, output=two)
    rec.one(rng, *lead, k, k, NEW, None, 2, p(two), S())
    out = fl.FoR.unfor_compare_range(0, empty, refs, 4, 4)
    assert out.numel() == 0
    rec.one(rng, *lead, k, k, NEW, None, 0, p(out), S())


@pytest.mark.parametrize("ty", TYS)
def test_width_zero_block_count_select_and_aggregate(fl, rec, ty):
    """unfor_select / unfor_aggregate: n_blocks, else the mask's 32-word blocks, else 0."""
    empty, refs, two, oo2, dst = col(ty, 0), col(ty, 1), words(2 * 32), longs(2), col(ty, 8)
    lead = (0, 0, p(refs), 0)
    fl.FoR.unfor_select(0, empty, refs, two, out_offsets=oo2, output=dst, n_blocks=2, check=False)
    rec.one(f"fl_{ty}_unfor_select", *lead, p(two), p(oo2), p(dst), 8, 2, None, S())
    fl.FoR.unfor_select(0, empty, refs, two, out_offsets=oo2, output=dst, check=False)
    rec.one(f"fl_{ty}_unfor_select", *lead, p(two), p(oo2), p(dst), 8, 2, None, S())
    with pytest.raises(ValueError):                                                       # n_blocks comes before the mask
        fl.FoR.unfor_select(0, empty, refs, two, out_offsets=oo2, output=dst, n_blocks=N, check=False)
    assert rec.take() == []
    agg = f"fl_{ty}_unfor_aggregate"
    result, slots = fl.FoR.unfor_aggregate(0, empty, refs, n_blocks=N, check=False)
    assert rec.take() == [(agg, (*lead, None, N, p(slots), None, S())), ("fl_aggregate_reduce", (p(slots), N, p(result), S()))]
    result, slots = fl.FoR.unfor_aggregate(0, empty, refs, two, check=False)
    assert rec.take() == [(agg, (*lead, p(two), 2, p(slots), None, S())), ("fl_aggregate_reduce", (p(slots), 2, p(result), S()))]
    result, slots = fl.FoR.unfor_aggregate(0, empty, refs, check=False)                   # none of them: 0 blocks
    assert tuple(slots.shape) == (0, 4)
    assert rec.take() == [(agg, (*lead, None, 0, None, None, S())), ("fl_aggregate_reduce", (None, 0, p(result), S()))]


@pytest.mark.parametrize("ty", TYS)
def test_zero_blocks_pass_null_mask_and_slots(fl, rec, ty):
    """No blocks: the mask_in pointer of the range forms, the mask and the slots of the aggregate forms arrive as NULL."""
    import torch
    empty, refs, nomask = col(ty, 0), col(ty, 1), words(0)
    k = (CT[ty], 1)
    out = fl.FoR.unfor_compare_range(W, empty, refs, 1, 1, mask=nomask, combine="and")
    rec.one(f"fl_{ty}_unfor_compare_range", W, 0, p(refs), 0, k, k, AND, None, 0, p(out), S())
    result, slots = fl.FoR.unfor_aggregate(W, empty, refs, nomask)
    assert rec.take() == [(f"fl_{ty}_unfor_aggregate", (W, 0, p(refs), 0, None, 0, None, PTR, S())),
                          ("fl_aggregate_reduce", (None, 0, p(result), S()))]
    w, o = torch.zeros(0, dtype=torch.uint8, device="cuda"), longs(0)
    out = fl.unfor_compare_range_widths(w, o, empty, refs, 1, 1, mask=nomask, combine="or", check=False)
    rec.one(f"fl_{ty}_unfor_compare_range_widths", 0, 0, 0, 0, p(refs), 0, k, k, OR, None, 0, p(out), None, S())
    result, slots = fl.unfor_aggregate_widths(w, o, empty, refs, nomask, check=False)
    assert rec.take() == [(f"fl_{ty}_unfor_aggregate_widths", (0, 0, 0, 0, p(refs), 0, None, 0, None, None, S())),
                          ("fl_aggregate_reduce", (None, 0, p(result), S()))]


def test_calls_go_to_the_current_stream(fl, rec):
    import torch
    ty = "u8"
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    pk, v, refs = col(ty, N * plen(ty, W)), col(ty, N * 1024), col(ty, N)
    w, o, mpk, nbytes = mixed(ty)
    b, _, _ = _batch(fl, ty, bases=[col(ty, N * 128) for _ in range(3)])
    plan = fl.MixedWidthPlan(ty, [0, 3, 8])
    try:
        with torch.cuda.stream(side):
            assert S() == side.cuda_stream
            fl.BitPacking.unpack(W, pk, v)
            fl.FoR.unfor_compare(W, pk, refs, "<", 1)
            fl.FoR.unfor_aggregate(W, pk, refs)
            fl.unpack_widths(w, o, mpk, v, check=False)
            fl.unfor_select_widths(w, o, mpk, refs, words(32 * N), out_offsets=longs(N), output=col(ty, 4))
            fl.widths_to_offsets(ty, w)
            fl.mask_offsets(words(32 * N))
            fl.for_widths(refs, refs)
            fl.BitPacking.unpack_single(W, pk, longs(2))
            fl.unpack_single_widths(w, o, mpk, longs(2))
            b.unpack()
            b.undelta_pack()
            plan.unpack(mpk, v)
            plan.pack(v, mpk)
        calls = rec.take()
        assert len(calls) == 15                                                           # unfor_aggregate is two launches
        assert [name for name, args in calls if args[-1] != side.cuda_stream] == []
        fl.BitPacking.unpack(W, pk, v)                                                    # and back on the default stream
        assert rec.take()[0][1][-1] == S() != side.cuda_stream
    finally:
        plan.close()
