"""GPU: unfor_aggregate_columns / unfor_aggregate_columns_widths -- COUNT / SUM / MIN / MAX of a * b, a + b or a - b between two
FoR-packed columns of one element type under a selection mask -- against the oracle's unfor_pack of both columns per block
(ffor.rs:38-50), combined with numpy in uint64 (both values zero-extended first, the operation wrapping mod 2^64) and reduced under the
mask's bits: per block {count, wrapping uint64 sum, min, max} of the uint64 patterns (nothing kept: {0, 0, 2^64 - 1, 0}), and numpy's
combination of the blocks.  Bit-exact.  Every case asserts on the REFERENCE that it exercises what it claims."""
import ctypes

import numpy as np
import pytest

from datagen import values
from oracle_lib import packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import IDENTITY, SENTINEL, TDT, TYS, combine, expected_blocks, mask_set, mask_words, mixed_column, sentinel_slots, to_dev, u64_of

pytestmark = pytest.mark.gpu

OPS = ["*", "+", "-"]
MIXED_BLOCKS = {"u8": 43, "u16": 67, "u32": 83, "u64": 163}            # T + 1 widths and a tail; none a multiple of 4


def expr(op, va, vb):
    """the definition: zero-extend, then the operation mod 2^64"""
    x, y = va.astype(np.uint64), vb.astype(np.uint64)
    with np.errstate(over="ignore"):
        return x * y if op == "*" else x + y if op == "+" else x - y


def decode(oracle, ty, blocks, refs):
    return np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])


def decodes_something(bits, wa, wb, n):
    """some block has a non-empty mask AND a packed row in either column: the decode path cannot be skipped wholesale"""
    kept = np.ones(n, bool) if bits is None else bits.reshape(n, 1024).any(axis=1)
    return bool((kept & ((np.asarray(wa) > 0) | (np.asarray(wb) > 0))).any())


def kept_rows(bits, size):
    return np.ones(size, bool) if bits is None else bits


def check_slots(buf, n, result, want, what):
    got = u64_of(buf)
    assert np.array_equal(got[:n * 4].reshape(n, 4), want), what
    assert (got[n * 4:] == SENTINEL).all(), (what, "the guard was written")
    assert np.array_equal(u64_of(result), combine(want)), (what, "result")


def wrapped_products(va, vb):
    x, y = va.astype(np.uint64), vb.astype(np.uint64)
    return (x != 0) & (expr("*", va, vb) // np.where(x == 0, np.uint64(1), x) != y)


@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_columns_every_op_and_mask(fl, oracle, ty):
    """Column a with the widths 0..T and a random tail against column b with T..0 and another tail -- every pair class (0,0), (0,w),
    (w,0), (T,T), (w,w') occurs; random wrapping per-block references and one broadcast reference per column; the three ops; the whole
    mask set (its one-bit-per-block masks: one element decides min and max) and no mask; slots pre-filled with a sentinel, the guard
    behind them untouched."""
    T = tbits(ty)
    n = MIXED_BLOCKS[ty]
    assert n % 4 and n > T + 3
    rng = np.random.default_rng(19100 + T)
    tail_a, tail_b = rng.integers(0, T + 1, size=n - (T + 1)), rng.integers(0, T + 1, size=n - (T + 1))
    tail_a[:4], tail_b[:4] = (0, T, 0, 3), (0, T, 2, 0)
    wa, wb = np.concatenate([np.arange(T + 1), tail_a]), np.concatenate([np.arange(T, -1, -1), tail_b])
    classes = {(min(a, 1) if a < T else 2, min(b, 1) if b < T else 2) for a, b in zip(wa.tolist(), wb.tolist())}
    assert {(0, 0), (0, 1), (1, 0), (2, 2), (1, 1), (0, 2), (2, 0)} <= classes
    assert ((wa > 0) & (wb > 0) & (wa != wb)).any()
    daw, daoff, acol, ablocks = mixed_column(ty, wa, 19200 + T)
    dbw, dboff, bcol, bblocks = mixed_column(ty, wb, 19300 + T)
    dacol, dbcol = to_dev(acol), to_dev(bcol)
    ra, rb = values(ty, n, 19400 + T), values(ty, n, 19500 + T)
    masks = mask_set(n, rng, with_none=True)
    for rname, ra_host, rb_host, dra, drb in (("per block", ra, rb, to_dev(ra), to_dev(rb)),
                                              ("broadcast", np.full(n, ra[3], dtype=ra.dtype), np.full(n, rb[5], dtype=rb.dtype), to_dev(ra[3:4]), to_dev(rb[5:6]))):
        va, vb = decode(oracle, ty, ablocks, ra_host), decode(oracle, ty, bblocks, rb_host)
        if rname == "per block":                                            # FoR's own add wraps mod 2^T somewhere in both columns
            assert (va < np.repeat(ra_host, 1024)).any() and (vb < np.repeat(rb_host, 1024)).any()
        for op in OPS:
            x = expr(op, va, vb)
            # witnesses, on the expected values
            if ty == "u64" and op == "*":
                assert wrapped_products(va, vb).any()
            if ty == "u64" and op == "+":
                assert (x < va).any()                                       # a sum below its summand: it wrapped
            if ty == "u32" and op == "*":
                assert (x >= np.uint64(1 << 32)).any()
            if ty == "u16" and op == "*":
                assert (expected_blocks(x, None)[:, 1] >= np.uint64(1 << 32)).any()   # a block sum past 32 bits
            for name, bits in masks.items():
                assert name == "zeros" or decodes_something(bits, wa, wb, n)
                if op == "-" and kept_rows(bits, x.size).reshape(n, 1024).any(axis=1).sum() > 1:   # (one block's two ranges may not cross)
                    assert (kept_rows(bits, x.size) & (va < vb)).any()      # a kept row below zero: its two's-complement pattern
                want = expected_blocks(x, bits)
                buf, slots = sentinel_slots(n)
                result, got = fl.unfor_aggregate_columns_widths(daw, daoff, dacol, dra, op, dbw, dboff, dbcol, drb,
                                                                mask=None if bits is None else mask_words(bits), block_aggs=slots)
                assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (n, 4) and tuple(result.shape) == (4,)
                check_slots(buf, n, result, want, (ty, rname, op, name))
        # the convenience path: the slots allocated inside the call
        result, got = fl.unfor_aggregate_columns_widths(daw, daoff, dacol, dra, "*", dbw, dboff, dbcol, drb, mask=mask_words(masks["random 1 %"]))
        want = expected_blocks(expr("*", va, vb), masks["random 1 %"])
        assert np.array_equal(u64_of(got), want) and np.array_equal(u64_of(result), combine(want)), (ty, rname, "block_aggs=None")


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_form(fl, oracle, ty):
    """61 blocks; every width of {0, 1, 3, T/2, T - 1, T} for column a against a different one of them for column b, and (0, 0) and
    (T, T); per-block references, and one zero reference with stride 0 on both sides: the plain bit-packed columns' expression"""
    T = tbits(ty)
    rng = np.random.default_rng(19600 + T)
    n = 61
    ws = sorted({0, 1, 3, T // 2, T - 1, T})
    pairs = [(w, ws[(i + 2) % len(ws)]) for i, w in enumerate(ws)] + [(0, 0), (T, T)]
    assert all(a != b for a, b in pairs[:-2]) and {a for a, _ in pairs} == set(ws)
    masks = mask_set(n, rng, full=False, with_none=True)
    ra, rb = values(ty, n, 19700 + T), values(ty, n, 19800 + T)
    dra, drb = to_dev(ra), to_dev(rb)
    for wa, wb in pairs:
        apk, bpk = values(ty, n * packed_len(ty, wa), 19900 + 64 * T + wa), values(ty, n * packed_len(ty, wb), 20000 + 64 * T + wb)
        va = oracle.batch("unfor_pack", ty, wa, apk, aux=ra, n_blocks=n)
        vb = oracle.batch("unfor_pack", ty, wb, bpk, aux=rb, n_blocks=n)
        pa, pb = oracle.batch("unpack", ty, wa, apk, n_blocks=n), oracle.batch("unpack", ty, wb, bpk, n_blocks=n)
        dapk, dbpk = to_dev(apk), to_dev(bpk)
        for op in OPS:
            x, plain = expr(op, va, vb), expr(op, pa, pb)
            for name, bits in masks.items():
                assert name == "zeros" or (wa == 0 and wb == 0) or decodes_something(bits, np.full(n, wa), np.full(n, wb), n)
                dm = None if bits is None else mask_words(bits)
                buf, slots = sentinel_slots(n)
                result, _ = fl.FoR.unfor_aggregate_columns(wa, dapk, dra, op, wb, dbpk, drb, mask=dm, n_blocks=n, block_aggs=slots)
                check_slots(buf, n, result, expected_blocks(x, bits), (ty, wa, wb, op, name))
                buf, slots = sentinel_slots(n)
                result, _ = fl.FoR.unfor_aggregate_columns(wa, dapk, 0, op, wb, dbpk, 0, mask=dm, n_blocks=n, block_aggs=slots)
                check_slots(buf, n, result, expected_blocks(plain, bits), (ty, wa, wb, op, name, "references 0"))
        if wa and wb:                                                       # the plain product is not trivially zero
            assert expr("*", pa, pb).any()


@pytest.mark.parametrize("ty", TYS)
def test_three_blocks_unlike_widths_and_strides_in_both_forms(fl, oracle, ty):
    """3 blocks, column a of width 5 against column b of width 3, one reference per block on one side and one broadcast reference on
    the other (then the other way round), a - b (which tells a from b) and a * b, through the uniform-width form and the mixed-width
    one.  The broadcast reference is the head of a longer tensor: a stride of 1 where 0 is meant reads other references, a column or a
    stride in the other's place changes the slots."""
    import torch
    T, n = tbits(ty), 3
    apk, bpk = values(ty, n * packed_len(ty, 5), 20100 + T), values(ty, n * packed_len(ty, 3), 20101 + T)
    ra, rb = values(ty, n, 20102 + T), values(ty, n, 20103 + T)
    assert len(set(ra.tolist())) == n and len(set(rb.tolist())) == n
    dapk, dbpk, dra, drb = to_dev(apk), to_dev(bpk), to_dev(ra), to_dev(rb)
    daw, dbw = (torch.full((n,), w, dtype=torch.uint8, device="cuda:0") for w in (5, 3))
    daoff, dboff = fl.widths_to_offsets(ty, daw)[0], fl.widths_to_offsets(ty, dbw)[0]
    bits = np.random.default_rng(20104 + T).random(n * 1024) < 0.6
    dm = mask_words(bits)
    for a_broadcast in (False, True):
        ha, hb = (np.full(n, ra[0]), rb) if a_broadcast else (ra, np.full(n, rb[0]))
        fa, fb = (dra[:1], drb) if a_broadcast else (dra, drb[:1])
        va = oracle.batch("unfor_pack", ty, 5, apk, aux=ha, n_blocks=n)
        vb = oracle.batch("unfor_pack", ty, 3, bpk, aux=hb, n_blocks=n)
        for op in ("-", "*"):
            want = expected_blocks(expr(op, va, vb), bits)
            buf, slots = sentinel_slots(n)
            result, _ = fl.FoR.unfor_aggregate_columns(5, dapk, fa, op, 3, dbpk, fb, mask=dm, n_blocks=n, block_aggs=slots)
            check_slots(buf, n, result, want, (ty, a_broadcast, op, "uniform"))
            buf, slots = sentinel_slots(n)
            result, _ = fl.unfor_aggregate_columns_widths(daw, daoff, dapk, fa, op, dbw, dboff, dbpk, fb, mask=dm, block_aggs=slots)
            check_slots(buf, n, result, want, (ty, a_broadcast, op, "mixed"))


@pytest.mark.parametrize("ty", TYS)
def test_consistent_with_the_shipped_aggregate(fl, oracle, ty):
    """A constant column b (width 0 in every block, no packed bytes): a * 1 and a + 0 equal unfor_aggregate_widths of column a, slot for
    slot; a - a is {count, 0, 0, 0} on every block that keeps something"""
    import torch
    T = tbits(ty)
    n = 53
    rng = np.random.default_rng(20100 + T)
    wa = np.concatenate([[0, T, 1], rng.integers(0, T + 1, size=n - 3)])
    daw, daoff, acol, ablocks = mixed_column(ty, wa, 20101)
    dacol = to_dev(acol)
    ra = values(ty, n, 20102)
    dra = to_dev(ra)
    z = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    one, zero = to_dev(np.ones(1, dtype=ra.dtype)), to_dev(np.zeros(1, dtype=ra.dtype))
    va = decode(oracle, ty, ablocks, ra)
    for name, bits in mask_set(n, rng, full=False, with_none=True).items():
        assert name == "zeros" or decodes_something(bits, wa, np.zeros(n), n)
        dm = None if bits is None else mask_words(bits)
        shipped_result, shipped = fl.unfor_aggregate_widths(daw, daoff, dacol, dra, dm)
        assert np.array_equal(u64_of(shipped), expected_blocks(va, bits))   # (the yardstick itself is right)
        for op, dref in (("*", one), ("+", zero)):
            result, got = fl.unfor_aggregate_columns_widths(daw, daoff, dacol, dra, op, z, zoff, empty, dref, mask=dm)
            assert torch.equal(got, shipped) and torch.equal(result, shipped_result), (ty, name, op)
            # ... and with the constant column on the left
            result, got = fl.unfor_aggregate_columns_widths(z, zoff, empty, dref, op, daw, daoff, dacol, dra, mask=dm)
            assert torch.equal(got, shipped) and torch.equal(result, shipped_result), (ty, name, op, "swapped")
        _, got = fl.unfor_aggregate_columns_widths(daw, daoff, dacol, dra, "-", daw, daoff, dacol, dra, mask=dm)
        count = expected_blocks(va, bits)[:, 0]
        want = np.where((count > 0)[:, None], np.stack([count, 0 * count, 0 * count, 0 * count], axis=1), IDENTITY[None, :])
        assert np.array_equal(u64_of(got), want), (ty, name, "a - a")
        assert name == "zeros" or (count > 0).any()


@pytest.mark.parametrize("ty", TYS)
def test_failing_blocks_flag_and_give_the_identity(fl, oracle, ty):
    """A width > T in column a only (block 7), a block outside the packed bytes in column b only (block 11): the flag carries both
    bits, the two slots hold the identity (not the sentinel: the slot feeds a reduction), every other slot and the total are right;
    check=False raises nothing, check=True raises."""
    import torch
    T = tbits(ty)
    esz = T // 8
    n = 40
    rng = np.random.default_rng(20200 + T)
    wa, wb = rng.integers(1, T + 1, size=n).astype(np.uint8), rng.integers(1, T + 1, size=n).astype(np.uint8)
    daw, daoff, acol, ablocks = mixed_column(ty, wa, 20201)
    dbw, dboff, bcol, bblocks = mixed_column(ty, wb, 20202)
    ra, rb = values(ty, n, 20203), values(ty, n, 20204)
    va, vb = decode(oracle, ty, ablocks, ra), decode(oracle, ty, bblocks, rb)
    bits = rng.random(n * 1024) < 0.2
    assert decodes_something(bits, wa, wb, n) and bits.reshape(n, 1024)[[7, 11]].any(axis=1).all()
    dm = mask_words(bits)
    bad_wa = wa.copy()
    bad_wa[7] = T + 1
    bad_boff = dboff.cpu().numpy().copy()
    bad_boff[11] += 1 << 40
    dbad_wa, dbad_boff = torch.from_numpy(bad_wa).cuda(), torch.from_numpy(bad_boff).cuda()
    dacol, dbcol, dra, drb = to_dev(acol), to_dev(bcol), to_dev(ra), to_dev(rb)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for code, op in enumerate(OPS):
        want = expected_blocks(expr(op, va, vb), bits)
        assert not np.array_equal(want[7], IDENTITY) and not np.array_equal(want[11], IDENTITY)
        want[[7, 11]] = IDENTITY
        buf, slots = sentinel_slots(n)
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = getattr(fl.load(), f"fl_{ty}_unfor_aggregate_columns_widths")(
            code, dbad_wa.data_ptr(), daoff.data_ptr(), dacol.data_ptr(), acol.size * esz, dra.data_ptr(), 1,
            dbw.data_ptr(), dbad_boff.data_ptr(), dbcol.data_ptr(), bcol.size * esz, drb.data_ptr(), 1,
            dm.data_ptr(), n, slots.data_ptr(), err.data_ptr(), stream)
        assert rc == 0
        assert int(err.item()) == 1 | 8, (ty, op, int(err.item()))
        check_slots(buf, n, fl.aggregate_reduce(slots), want, (ty, op))
        # the Python form: asynchronous and silent with check=False, the same slots and total
        buf, slots = sentinel_slots(n)
        result, _ = fl.unfor_aggregate_columns_widths(dbad_wa, daoff, dacol, dra, op, dbw, dbad_boff, dbcol, drb, mask=dm, block_aggs=slots, check=False)
        check_slots(buf, n, result, want, (ty, op, "check=False"))
    for status, aw_, bo_ in ((1, dbad_wa, dboff), (6, daw, dbad_boff)):
        with pytest.raises(fl.FastLanesError) as ei:
            fl.unfor_aggregate_columns_widths(aw_, daoff, dacol, dra, "*", dbw, bo_, dbcol, drb, mask=dm)
        assert ei.value.status == status, (ty, status)
    with pytest.raises(fl.FastLanesError):
        fl.unfor_aggregate_columns_widths(dbad_wa, daoff, dacol, dra, "*", dbw, dbad_boff, dbcol, drb, mask=dm)


def test_q6_shape_end_to_end(fl, oracle):
    """SELECT SUM(price * discount) WHERE shipdate BETWEEN a AND b AND discount BETWEEN c AND d: two range masks chained with AND, the
    aggregate of the product under them, four u32 columns' worth of nothing materialised -- against numpy over the oracle's decode"""
    ty, T, n = "u32", 32, 41
    rng = np.random.default_rng(20300)
    cols = {}
    for i, name in enumerate(("shipdate", "discount", "price")):
        dw, doff, col, blocks = mixed_column(ty, rng.integers(0, T + 1, size=n), 20301 + i)
        refs = values(ty, n, 20311 + i)
        cols[name] = ((dw, doff, to_dev(col), to_dev(refs)), decode(oracle, ty, blocks, refs))
    ship, disc, price = (cols[k][1] for k in ("shipdate", "discount", "price"))
    a, b = (int(q) for q in np.quantile(ship, [0.2, 0.7]).astype(np.uint64))
    c, d = (int(q) for q in np.quantile(disc, [0.1, 0.8]).astype(np.uint64))
    m = fl.unfor_compare_range_widths(*cols["shipdate"][0], a, b)
    m = fl.unfor_compare_range_widths(*cols["discount"][0], c, d, mask=m, combine="and", output=m)
    keep = (ship >= a) & (ship <= b) & (disc >= c) & (disc <= d)
    x = expr("*", price, disc)
    kept = x[keep]
    assert 0.1 * keep.size < kept.size < 0.6 * keep.size and (kept >= np.uint64(1 << 32)).any()
    result, slots = fl.unfor_aggregate_columns_widths(*cols["price"][0], "*", *cols["discount"][0], mask=m)
    want = expected_blocks(x, keep)
    assert np.array_equal(u64_of(slots), want)
    assert [int(v) for v in u64_of(result)] == [kept.size, int(kept.sum(dtype=np.uint64)), int(kept.min()), int(kept.max())]


@pytest.mark.parametrize("policy", [2 + 256 * 4 + 65536 * 4 + (1 << 24), 2 + 256 * 4 + 65536 * 2 + (1 << 24), 2 + 256 * 6 + 65536 * 3])
@pytest.mark.parametrize("ty", TYS)
def test_launch_shapes_streams_and_empty_columns(fl, oracle, kernel_policy, ty, policy):
    """Forced launch shapes -- 4 and 2 blocks per wavefront with prefetch (the narrow types' shipped shapes), 3 without -- on 67 blocks,
    both forms on a non-default stream; empty columns; columns of width-0 blocks with no packed bytes on either side"""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    n = 67
    rng = np.random.default_rng(20400 + T)
    wa, wb = rng.integers(0, T + 1, size=n), rng.integers(0, T + 1, size=n)
    daw, daoff, acol, ablocks = mixed_column(ty, wa, 20401)
    dbw, dboff, bcol, bblocks = mixed_column(ty, wb, 20402)
    ra, rb = values(ty, n, 20403), values(ty, n, 20404)
    va, vb = decode(oracle, ty, ablocks, ra), decode(oracle, ty, bblocks, rb)
    w2a, w2b = T // 2, T // 2 + 1
    pk2a, pk2b = values(ty, n * packed_len(ty, w2a), 20405), values(ty, n * packed_len(ty, w2b), 20406)
    v2a = oracle.batch("unfor_pack", ty, w2a, pk2a, aux=ra, n_blocks=n)
    v2b = oracle.batch("unfor_pack", ty, w2b, pk2b, aux=rb, n_blocks=n)
    dacol, dbcol, dra, drb, dpk2a, dpk2b = (to_dev(x) for x in (acol, bcol, ra, rb, pk2a, pk2b))
    s = torch.cuda.Stream()
    masks = mask_set(n, rng, full=False, with_none=True)
    for i, (name, bits) in enumerate(masks.items()):
        op = OPS[i % 3]
        assert name == "zeros" or decodes_something(bits, wa, wb, n)
        dm = None if bits is None else mask_words(bits)
        (buf1, slots1), (buf2, slots2) = sentinel_slots(n), sentinel_slots(n)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            r1, _ = fl.unfor_aggregate_columns_widths(daw, daoff, dacol, dra, op, dbw, dboff, dbcol, drb, mask=dm, block_aggs=slots1, check=False)
            r2, _ = fl.FoR.unfor_aggregate_columns(w2a, dpk2a, dra, op, w2b, dpk2b, drb, mask=dm, block_aggs=slots2)
        s.synchronize()
        check_slots(buf1, n, r1, expected_blocks(expr(op, va, vb), bits), (ty, policy, op, name))
        check_slots(buf2, n, r2, expected_blocks(expr(op, v2a, v2b), bits), (ty, policy, op, name, "uniform"))
    # empty columns: the identity
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    ew, eo = torch.empty(0, dtype=torch.uint8, device="cuda:0"), torch.empty(0, dtype=torch.int64, device="cuda:0")
    for m in (torch.empty(0, dtype=torch.int32, device="cuda:0"), None):
        result, slots = fl.unfor_aggregate_columns_widths(ew, eo, empty, dra[:1], "*", ew, eo, empty, drb[:1], mask=m)
        assert tuple(slots.shape) == (0, 4) and np.array_equal(u64_of(result), IDENTITY)
        result, slots = fl.FoR.unfor_aggregate_columns(3, empty, 0, "+", 5, empty, 0, mask=m)
        assert tuple(slots.shape) == (0, 4) and np.array_equal(u64_of(result), IDENTITY)
    # width-0 blocks on both sides, no packed bytes at all: every row holds ra o rb, the count comes from the mask alone
    z = torch.zeros(5, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    bits = rng.random(5 * 1024) < 0.4
    za, zb = np.repeat(ra[:5], 1024), np.repeat(rb[:5], 1024)
    for op in OPS:
        for b_ in (bits, None):
            want = expected_blocks(expr(op, za, zb), b_)
            dm = None if b_ is None else mask_words(b_)
            result, slots = fl.unfor_aggregate_columns_widths(z, zoff, empty, dra[:5], op, z, zoff, empty, drb[:5], mask=dm)
            assert np.array_equal(u64_of(slots), want) and np.array_equal(u64_of(result), combine(want)), (ty, policy, op, "width 0")
            result, slots = fl.FoR.unfor_aggregate_columns(0, empty, dra[:5], op, 0, empty, drb[:5], mask=dm, n_blocks=5)
            assert np.array_equal(u64_of(slots), want) and np.array_equal(u64_of(result), combine(want)), (ty, policy, op, "uniform width 0")
