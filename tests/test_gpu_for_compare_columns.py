"""GPU: unfor_compare_columns / unfor_compare_columns_widths -- a <op> b between two FoR-packed columns of one element type, chained
through a mask -- against the mask numpy builds from the oracle's unfor_pack of both columns per block (ffor.rs:38-50):
    hit = va <op> vb (signed: on the signed view of the dtype);   new: hit,  and: mask_in & hit,  or: mask_in | hit
in unpack_compare's layout (bit i of word i // 32 of block b, LSB first).  Masks are compared bit for bit."""
import numpy as np
import pytest

from datagen import values
from oracle_lib import TYPES, packed_len, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TDT, TYS, got_mask, mixed_column, to_dev
from columns_data import ALL, EACH, MIRROR, NONE, ONE_BIT, OPS, columns_verdict, incoming_mask, pair_references, want_mask

pytestmark = pytest.mark.gpu

COMBINE = ["new", "and", "or"]
ORDERING = ["<", "<=", ">", ">="]
PREFILL = 0x5A5A5A5A
RAGGED = 263                            # blocks of the ragged column pair
SAME_REF, OTHER_REF = 8, 12             # its two block pairs with both widths 0: equal / different references


def prefilled(n):
    import torch
    return torch.full((n * 32,), PREFILL, dtype=torch.int32, device="cuda:0")


def decode(oracle, ty, blocks, refs):
    return np.concatenate([oracle.unfor_pack(ty, w, pk, refs[b]) for b, (w, pk) in enumerate(blocks)])


def column_pair(ty, n, seed):
    """widths of the two columns and their references by pair_references' recipe; the ragged pair carries the two width-0 pairs"""
    T = tbits(ty)
    rng = np.random.default_rng(seed)
    small = {1: ([T // 2], [T]), 2: ([3, T], [T - 1, 0]), 3: ([T, 0, 1], [2, 5, T]), 5: ([2, T - 1, 0, T, 5], [T, 1, 3, 0, T // 2])}
    if n == T + 1:
        wa, wb = np.arange(T + 1), rng.permutation(T + 1)
    elif n in small:
        wa, wb = (np.array(w) for w in small[n])
    else:
        wa, wb = rng.integers(0, T + 1, size=n), rng.integers(0, T + 1, size=n)
    if n == RAGGED:
        wa[[SAME_REF, OTHER_REF]] = 0
        wb[[SAME_REF, OTHER_REF]] = 0
    ra, rb = pair_references(T, wa, wb, seed + 1, TYPES[ty][0])
    if n == RAGGED:
        rb[SAME_REF] = ra[SAME_REF]
        rb[OTHER_REF] = ra[OTHER_REF] + ra.dtype.type(5)
    return wa, wb, ra, rb


@pytest.mark.parametrize("ty", TYS)
def test_mixed_width_columns_every_op_and_combiner(fl, oracle, ty):
    """Column a with every width 0..T against a permutation of them, a ragged pair of 263 blocks, and 1 / 2 / 3 / 5 blocks; the
    references overlap the two ranges except where b % 4 == 1 (a < b everywhere) and b % 4 == 3 (a > b everywhere), plus one pair of
    constant blocks with equal and one with different references.  Six ops x unsigned / signed x the three combiners over incoming
    masks that mix random blocks with empty, full, one-bit-set and one-bit-clear ones; out of place into an output prefilled with 0x5A
    bytes, and in place; per-block references and one broadcast reference on either side.  The 263-block column must hold, by this
    file's own restatement of the rule, at least a third undecided blocks and both ALL and NONE for every ordering op, ALL and NONE from
    the width-0 pairs for == / !=, and at least half of the ordering ops' undecided blocks with a mask that is neither empty nor full
    (== between random wide values is empty whatever the recipe)."""
    T = tbits(ty)
    with np.errstate(over="ignore"):
        for n in (T + 1, RAGGED, 1, 2, 3, 5):
            wa, wb, ra, rb = column_pair(ty, n, 11000 + 64 * T + n)
            daw, daoff, acol, ablocks = mixed_column(ty, wa, 11100 + n)
            dbw, dboff, bcol, bblocks = mixed_column(ty, wb, 11200 + n)
            dacol, dbcol = to_dev(acol), to_dev(bcol)
            kinds = [("per block", ra, rb, to_dev(ra), to_dev(rb))]
            if n >= T + 1:
                mid = n // 2
                kinds.append(("broadcast a", np.full(n, ra[mid], dtype=ra.dtype), rb, to_dev(ra[mid:mid + 1]), to_dev(rb)))
                kinds.append(("broadcast b", ra, np.full(n, rb[mid], dtype=rb.dtype), to_dev(ra), to_dev(rb[mid:mid + 1])))
            for rname, ra_h, rb_h, dra, drb in kinds:
                va, vb = decode(oracle, ty, ablocks, ra_h), decode(oracle, ty, bblocks, rb_h)
                q = 0
                for signed in (False, True):
                    for op in OPS:
                        hit = want_mask(va, vb, op, signed).reshape(n, 32)
                        if n == RAGGED and rname == "per block":
                            v = np.array([columns_verdict(T, op, signed, int(ra_h[b]), int(wa[b]), int(rb_h[b]), int(wb[b])) for b in range(n)])
                            if op in ORDERING:
                                assert 3 * (v == EACH).sum() >= n and (v == ALL).any() and (v == NONE).any(), (ty, op, signed, np.bincount(v))
                                open_masks = hit[v == EACH]
                                mixed = ((open_masks != 0).any(axis=1) & (open_masks != -1).any(axis=1)).sum()
                                assert 2 * mixed >= (v == EACH).sum(), (ty, op, signed, mixed, (v == EACH).sum())
                            else:
                                assert {v[SAME_REF], v[OTHER_REF]} == {ALL, NONE} and v[SAME_REF] == (ALL if op == "==" else NONE), (ty, op)
                            assert (hit[v == ALL] == -1).all() and (hit[v == NONE] == 0).all()     # the restatement agrees with the values
                        min_host = incoming_mask(n, 11300 + n, shift=q)
                        q += 1
                        dmin = to_dev(min_host)
                        for cb in COMBINE:
                            want = want_mask(va, vb, op, signed, cb, min_host)
                            args = dict(mask=dmin, combine=cb) if cb != "new" else {}
                            got = got_mask(fl.unfor_compare_columns_widths(daw, daoff, dacol, dra, op, dbw, dboff, dbcol, drb, signed=signed,
                                                                           output=prefilled(n), **args))
                            assert np.array_equal(got, want), (ty, n, rname, op, signed, cb)
                            if cb != "new":
                                inplace = dmin.clone()
                                out = fl.unfor_compare_columns_widths(daw, daoff, dacol, dra, op, dbw, dboff, dbcol, drb, signed=signed,
                                                                      mask=inplace, combine=cb, output=inplace)
                                assert out is inplace and np.array_equal(got_mask(inplace), want), (ty, n, rname, op, signed, cb, "in place")
                                assert np.array_equal(got_mask(dmin), min_host)             # out of place left mask_in alone
                # "new" ignores a mask it is given
                got = got_mask(fl.unfor_compare_columns_widths(daw, daoff, dacol, dra, "<", dbw, dboff, dbcol, drb, mask=dmin, combine="new"))
                assert np.array_equal(got, want_mask(va, vb, "<", False)), (ty, n, rname, "new with a mask")


@pytest.mark.parametrize("ty", TYS)
def test_one_element_decides(fl, oracle, ty):
    """Column b decodes to exactly column a (the same packed bytes, widths and references): == is all ones, < all zeros, every block
    undecided.  Then pairs whose decoded values differ in exactly ONE element per block -- at the block's ends, the ends of the 16-byte
    mask slices, the first and last index of a lane's cell in the first and a later 1-KiB group -- by + 1, by - 1, and in the top bit
    only (signed and unsigned disagree); half of the pairs reach the same values from a shifted reference."""
    T = tbits(ty)
    dt = TYPES[ty][0]
    N = 1 << T
    rng = np.random.default_rng(11400 + T)
    n = 3 * len(ONE_BIT)
    widths = np.array([T if j % 3 == 2 else 2 + (j * 5) % (T - 1) for j in range(n)])
    dw, doff, col, blocks = mixed_column(ty, widths, 11401)
    refs = values(ty, n, 11402)
    dcol, drefs = to_dev(col), to_dev(refs)
    va = decode(oracle, ty, blocks, refs)
    for signed in (False, True):
        for op in OPS:
            assert {columns_verdict(T, op, signed, int(refs[b]), int(widths[b]), int(refs[b]), int(widths[b])) for b in range(n)} == {EACH}
            got = got_mask(fl.unfor_compare_columns_widths(dw, doff, dcol, drefs, op, dw, doff, dcol, drefs, signed=signed, output=prefilled(n)))
            assert (got == (-1 if op in ("==", "<=", ">=") else 0)).all(), (ty, op, signed, "a against itself")
    # one differing element per block: fields of column a in [1, 2^W - 3] (W = 2: 1), so that +- 1 and a reference one lower still fit
    fa = np.empty((n, 1024), dtype=np.uint64)
    fb = np.empty((n, 1024), dtype=np.uint64)
    rb = refs.copy()
    pieces_a, pieces_b = [], []
    with np.errstate(over="ignore"):
        for j in range(n):
            w, at, kind = int(widths[j]), ONE_BIT[j // 3], j % 3
            top = (1 << w) - 1
            fa[j] = rng.integers(1, max(top - 2, 1), size=1024, dtype=np.uint64, endpoint=True)
            fb[j] = fa[j]
            if kind == 2:
                fb[j, at] ^= np.uint64(1 << (T - 1))                        # W = T: the top bit only
            else:
                fb[j, at] += np.uint64(1) if kind == 0 else np.uint64(N - 1) if T < 64 else np.uint64(2 ** 64 - 1)
                fb[j, at] &= np.uint64(N - 1)
                if j % 2 and w < T:
                    rb[j] = refs[j] - dt(1)                            # the same values from a reference one lower
                    fb[j] += np.uint64(1)
            pieces_a.append(oracle.for_pack(ty, w, (fa[j].astype(dt) + refs[j]), refs[j]))
            pieces_b.append(oracle.for_pack(ty, w, (fb[j].astype(dt) + rb[j]), rb[j]))
    acol, bcol = np.concatenate(pieces_a), np.concatenate(pieces_b)
    assert acol.size == col.size and bcol.size == col.size
    a_blocks = [(w, pk) for (w, _), pk in zip(blocks, pieces_a)]
    b_blocks = [(w, pk) for (w, _), pk in zip(blocks, pieces_b)]
    va, vb = decode(oracle, ty, a_blocks, refs), decode(oracle, ty, b_blocks, rb)
    differ = (va != vb).reshape(n, 1024)
    assert (differ.sum(axis=1) == 1).all() and [int(np.flatnonzero(d)[0]) for d in differ] == [ONE_BIT[j // 3] for j in range(n)]
    dacol, dbcol, drb = to_dev(acol), to_dev(bcol), to_dev(rb)
    disagree = 0
    for op in OPS:
        w_unsigned = want_mask(va, vb, op, False)
        w_signed = want_mask(va, vb, op, True)
        disagree += int((w_unsigned != w_signed).sum())
        for signed, want in ((False, w_unsigned), (True, w_signed)):
            got = got_mask(fl.unfor_compare_columns_widths(dw, doff, dacol, drefs, op, dw, doff, dbcol, drb, signed=signed, output=prefilled(n)))
            assert np.array_equal(got, want), (ty, op, signed)
            got = got_mask(fl.unfor_compare_columns_widths(dw, doff, dbcol, drb, MIRROR[op], dw, doff, dacol, drefs, signed=signed))
            assert np.array_equal(got, want), (ty, op, signed, "swapped")
    assert disagree > 0                                                     # the top-bit pairs tell signed from unsigned


@pytest.mark.parametrize("ty", TYS)
def test_a_constant_side_equals_unfor_compare_widths(fl, oracle, ty):
    """Column b all width-0 blocks with one broadcast reference k: unfor_compare_widths(a, op, k), bit for bit, for the six ops; and
    with the columns swapped and the op mirrored."""
    import torch
    T = tbits(ty)
    M = (1 << T) - 1
    rng = np.random.default_rng(11500 + T)
    n = 70
    widths = rng.integers(0, T + 1, size=n)
    dw, doff, col, blocks = mixed_column(ty, widths, 11501)
    refs = values(ty, n, 11502)
    dcol, drefs = to_dev(col), to_dev(refs)
    z = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    zoff = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    top = (1 << int(widths[7])) - 1
    for k in (0, M, int(refs[7]), (int(refs[7]) + top) % (M + 1), (int(refs[7]) + top + 1) % (M + 1), int(refs[40]) ^ 5):
        dk = to_dev(np.array([k], dtype=TYPES[ty][0]))
        for op in OPS:
            old = got_mask(fl.unfor_compare_widths(dw, doff, dcol, drefs, op, k))
            got = got_mask(fl.unfor_compare_columns_widths(dw, doff, dcol, drefs, op, z, zoff, empty, dk, output=prefilled(n)))
            assert np.array_equal(got, old), (ty, op, k)
            got = got_mask(fl.unfor_compare_columns_widths(z, zoff, empty, dk, MIRROR[op], dw, doff, dcol, drefs, output=prefilled(n)))
            assert np.array_equal(got, old), (ty, op, k, "swapped")


@pytest.mark.parametrize("ty", TYS)
def test_uniform_width_every_width_pair(fl, oracle, ty):
    """FoR.unfor_compare_columns over uniform-width columns of 37 blocks: every W_a in 0..T against W_b in {0, 1, T/2, T - 1, T},
    per-block and scalar references, the three combiners, one in-place run per W_a"""
    T = tbits(ty)
    n = 37
    for wa in range(T + 1):
        apk = values(ty, n * packed_len(ty, wa), 11600 + 64 * T + wa)
        dapk = to_dev(apk)
        for i, wb in enumerate((0, 1, T // 2, T - 1, T)):
            bpk = values(ty, n * packed_len(ty, wb), 11700 + 64 * T + wb)
            ra, rb = pair_references(T, [wa] * n, [wb] * n, 11800 + 64 * wa + wb, TYPES[ty][0])
            va = oracle.batch("unfor_pack", ty, wa, apk, aux=ra, n_blocks=n)
            vb = oracle.batch("unfor_pack", ty, wb, bpk, aux=rb, n_blocks=n)
            dbpk, dra, drb = to_dev(bpk), to_dev(ra), to_dev(rb)
            op, signed = OPS[(wa + i) % 6], bool((wa + i // 2) % 2)
            min_host = incoming_mask(n, 11900 + wa, shift=wa + i)
            dmin = to_dev(min_host)
            for cb in COMBINE:
                args = dict(mask=dmin, combine=cb) if cb != "new" else {}
                got = got_mask(fl.FoR.unfor_compare_columns(wa, dapk, dra, op, wb, dbpk, drb, signed=signed, n_blocks=n, output=prefilled(n), **args))
                assert np.array_equal(got, want_mask(va, vb, op, signed, cb, min_host)), (ty, wa, wb, op, signed, cb)
            if i == wa % 5:
                inplace = dmin.clone()
                out = fl.FoR.unfor_compare_columns(wa, dapk, dra, op, wb, dbpk, drb, signed=signed, mask=inplace, combine="or", output=inplace)
                assert out is inplace and np.array_equal(got_mask(inplace), want_mask(va, vb, op, signed, "or", min_host)), (ty, wa, wb, "in place")
            # one scalar reference per column (reference_stride 0)
            sa, sb = int(ra[1]), int(rb[1])
            va0 = oracle.batch("unfor_pack", ty, wa, apk, aux=np.full(n, sa, dtype=ra.dtype), n_blocks=n)
            vb0 = oracle.batch("unfor_pack", ty, wb, bpk, aux=np.full(n, sb, dtype=rb.dtype), n_blocks=n)
            got = got_mask(fl.FoR.unfor_compare_columns(wa, dapk, sa, op, wb, dbpk, sb, signed=signed, mask=dmin, combine="and", n_blocks=n))
            assert np.array_equal(got, want_mask(va0, vb0, op, signed, "and", min_host)), (ty, wa, wb, "scalar references")


@pytest.mark.parametrize("ty", TYS)
def test_three_blocks_unlike_widths_and_strides_in_both_forms(fl, oracle, ty):
    """3 blocks, column a of width 5 against column b of width 3, one reference per block on one side and one broadcast reference on
    the other (then the other way round), all six ops -- those the entry point serves by swapping the columns among them -- through the
    uniform-width form and the mixed-width one.  The broadcast reference is the head of a longer tensor: a stride of 1 where 0 is meant
    reads other references, a column or a stride in the other's place changes the mask."""
    import torch
    T, n = tbits(ty), 3
    apk, bpk = values(ty, n * packed_len(ty, 5), 12400 + T), values(ty, n * packed_len(ty, 3), 12401 + T)
    r = int(values(ty, 1, 12402 + T)[0])                                    # every pair of ranges overlaps, whichever references meet
    ra, rb = (np.array([(r + d) % (1 << T) for d in ds], dtype=TYPES[ty][0]) for ds in ((0, 4, 8), (6, 12, 2)))
    dapk, dbpk, dra, drb = to_dev(apk), to_dev(bpk), to_dev(ra), to_dev(rb)
    daw, dbw = (torch.full((n,), w, dtype=torch.uint8, device="cuda:0") for w in (5, 3))
    daoff, dboff = fl.widths_to_offsets(ty, daw)[0], fl.widths_to_offsets(ty, dbw)[0]
    min_host = incoming_mask(n, 12403 + T)
    dmin = to_dev(min_host)
    for a_broadcast in (False, True):
        ha, hb = (np.full(n, ra[0]), rb) if a_broadcast else (ra, np.full(n, rb[0]))
        fa, fb = (dra[:1], drb) if a_broadcast else (dra, drb[:1])
        va = oracle.batch("unfor_pack", ty, 5, apk, aux=ha, n_blocks=n)
        vb = oracle.batch("unfor_pack", ty, 3, bpk, aux=hb, n_blocks=n)
        for i, op in enumerate(OPS):
            signed, cb = bool(i % 2), COMBINE[i % 3]
            want = want_mask(va, vb, op, signed, cb, min_host)
            args = dict(mask=dmin, combine=cb) if cb != "new" else {}
            got = got_mask(fl.FoR.unfor_compare_columns(5, dapk, fa, op, 3, dbpk, fb, signed=signed, n_blocks=n, output=prefilled(n), **args))
            assert np.array_equal(got, want), (ty, a_broadcast, op, signed, cb, "uniform")
            got = got_mask(fl.unfor_compare_columns_widths(daw, daoff, dapk, fa, op, dbw, dboff, dbpk, fb, signed=signed, output=prefilled(n), **args))
            assert np.array_equal(got, want), (ty, a_broadcast, op, signed, cb, "mixed")


@pytest.mark.parametrize("ty", TYS)
def test_device_checks_on_both_columns(fl, oracle, ty):
    """A width > T in column a (block 7), a misaligned offset in column b (block 5), a block outside the packed bytes in both (block
    11): err_flag holds the three bits, the three blocks keep their prefill, every other block is right under each combiner, and
    check=True raises the matching status."""
    import ctypes
    import torch
    T = tbits(ty)
    esz = T // 8
    n = 40
    rng = np.random.default_rng(12100 + T)
    wa, wb = rng.integers(1, T + 1, size=n).astype(np.uint8), rng.integers(1, T + 1, size=n).astype(np.uint8)
    daw, daoff, acol, ablocks = mixed_column(ty, wa, 12101)
    dbw, dboff, bcol, bblocks = mixed_column(ty, wb, 12102)
    ra, rb = pair_references(T, wa, wb, 12103, TYPES[ty][0])
    va, vb = decode(oracle, ty, ablocks, ra), decode(oracle, ty, bblocks, rb)
    aoff, boff = daoff.cpu().numpy(), dboff.cpu().numpy()
    bad_wa = wa.copy()
    bad_wa[7] = T + 1
    bad_aoff, bad_boff = aoff.copy(), boff.copy()
    bad_boff[5] += 8
    bad_aoff[11] += 1 << 40
    bad_boff[11] += 1 << 40
    cu = lambda a: torch.from_numpy(a).cuda()                               # noqa: E731
    dbad_wa, dbad_aoff, dbad_boff = cu(bad_wa), cu(bad_aoff), cu(bad_boff)
    dacol, dbcol, dra, drb = to_dev(acol), to_dev(bcol), to_dev(ra), to_dev(rb)
    lib = fl.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    min_host = incoming_mask(n, 12104)
    dmin = to_dev(min_host)
    skipped = np.zeros(n, dtype=bool)
    skipped[[5, 7, 11]] = True
    for code, cb in enumerate(COMBINE):
        op, signed = OPS[2 + code], code == 1
        mask = prefilled(n)
        err = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        rc = getattr(lib, f"fl_{ty}_unfor_compare_columns_widths")(
            dbad_wa.data_ptr(), dbad_aoff.data_ptr(), dacol.data_ptr(), acol.size * esz, dra.data_ptr(), 1,
            dbw.data_ptr(), dbad_boff.data_ptr(), dbcol.data_ptr(), bcol.size * esz, drb.data_ptr(), 1,
            2 + code, int(signed), code, dmin.data_ptr() if code else None, n, mask.data_ptr(), err.data_ptr(), stream)
        assert rc == 0
        assert int(err.item()) == 1 | 4 | 8, (ty, cb, int(err.item()))
        g = got_mask(mask).reshape(n, 32)
        w = want_mask(va, vb, op, signed, cb, min_host).reshape(n, 32)
        assert (g[skipped] == PREFILL).all(), (ty, cb, "a skipped block was written")
        assert np.array_equal(g[~skipped], w[~skipped]), (ty, cb)
    for status, aw_, ao_, bo_ in ((1, dbad_wa, daoff, dboff), (4, daw, daoff, cu(np.where(np.arange(n) == 5, boff + 8, boff))),
                                  (6, daw, cu(np.where(np.arange(n) == 11, aoff + (1 << 40), aoff)), cu(np.where(np.arange(n) == 11, boff + (1 << 40), boff)))):
        with pytest.raises(fl.FastLanesError) as ei:
            fl.unfor_compare_columns_widths(aw_, ao_, dacol, dra, "<", dbw, bo_, dbcol, drb, mask=dmin, combine="and")
        assert ei.value.status == status, (ty, status)


@pytest.mark.parametrize("policy", [0, 1, 2, 2 + 256 * 4 + 65536 * 4 + (1 << 24), 2 + 256 * 6 + 65536 * 3, 2 + 256 * 4 + 65536 * 12 + (1 << 24)])
@pytest.mark.parametrize("ty", TYS)
def test_policies_streams_and_empty_columns(fl, oracle, kernel_policy, ty, policy):
    """Kernel policies 0 / 1 / 2 (and forced waves / blocks per wavefront / prefetch, up to 12 blocks per wavefront) on 131 blocks, a
    non-default stream, empty columns and columns of width-0 blocks with no packed bytes."""
    import torch
    kernel_policy(policy)
    T = tbits(ty)
    n = 131
    wa, wb, ra, rb = column_pair(ty, n, 12200 + T)
    daw, daoff, acol, ablocks = mixed_column(ty, wa, 12201)
    dbw, dboff, bcol, bblocks = mixed_column(ty, wb, 12202)
    va, vb = decode(oracle, ty, ablocks, ra), decode(oracle, ty, bblocks, rb)
    w2a, w2b = T // 2, T // 2 + 1
    pk2a, pk2b = values(ty, n * packed_len(ty, w2a), 12203), values(ty, n * packed_len(ty, w2b), 12204)
    v2a = oracle.batch("unfor_pack", ty, w2a, pk2a, aux=ra, n_blocks=n)
    v2b = oracle.batch("unfor_pack", ty, w2b, pk2b, aux=rb, n_blocks=n)
    min_host = incoming_mask(n, 12205)
    s = torch.cuda.Stream()
    dacol, dbcol, dra, drb, dpk2a, dpk2b, dmin = (to_dev(x) for x in (acol, bcol, ra, rb, pk2a, pk2b, min_host))
    torch.cuda.synchronize()
    for i, cb in enumerate(COMBINE):
        op, signed = OPS[(2 * i + policy) % 6], bool(i % 2)
        args = dict(mask=dmin, combine=cb) if cb != "new" else {}
        inplace = dmin.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            m1 = fl.unfor_compare_columns_widths(daw, daoff, dacol, dra, op, dbw, dboff, dbcol, drb, signed=signed, check=False, output=prefilled(n), **args)
            m2 = fl.FoR.unfor_compare_columns(w2a, dpk2a, dra, op, w2b, dpk2b, drb, signed=signed, output=prefilled(n), **args)
            if cb != "new":
                fl.unfor_compare_columns_widths(daw, daoff, dacol, dra, op, dbw, dboff, dbcol, drb, signed=signed, mask=inplace, combine=cb,
                                                output=inplace, check=False)
        s.synchronize()
        assert np.array_equal(got_mask(m1), want_mask(va, vb, op, signed, cb, min_host)), (ty, policy, op, signed, cb)
        assert np.array_equal(got_mask(m2), want_mask(v2a, v2b, op, signed, cb, min_host)), (ty, policy, op, signed, cb, "uniform")
        if cb != "new":
            assert np.array_equal(got_mask(inplace), want_mask(va, vb, op, signed, cb, min_host)), (ty, policy, op, signed, cb, "in place")
    # empty columns
    empty = torch.empty(0, dtype=getattr(torch, TDT[ty]), device="cuda:0")
    nomask = torch.empty(0, dtype=torch.int32, device="cuda:0")
    ew, eo = torch.empty(0, dtype=torch.uint8, device="cuda:0"), torch.empty(0, dtype=torch.int64, device="cuda:0")
    assert fl.unfor_compare_columns_widths(ew, eo, empty, dra[:1], "<", ew, eo, empty, drb[:1]).numel() == 0
    assert fl.unfor_compare_columns_widths(ew, eo, empty, dra[:1], "<", ew, eo, empty, drb[:1], mask=nomask, combine="and").numel() == 0
    assert fl.FoR.unfor_compare_columns(3, empty, 0, "==", 5, empty, 0).numel() == 0
    # width-0 blocks, no packed bytes on either side: every value is its block's reference
    z = torch.zeros(5, dtype=torch.uint8, device="cuda:0")
    zoff, _ = fl.widths_to_offsets(ty, z)
    za, zb = np.repeat(ra[:5], 1024), np.repeat(rb[:5], 1024)
    mz = incoming_mask(5, 12206, shift=1)
    got = got_mask(fl.unfor_compare_columns_widths(z, zoff, empty, dra[:5], "<=", z, zoff, empty, drb[:5], signed=True, mask=to_dev(mz), combine="or"))
    assert np.array_equal(got, want_mask(za, zb, "<=", True, "or", mz)), (ty, policy, "width 0")
    got = got_mask(fl.FoR.unfor_compare_columns(0, empty, dra[:5], "!=", 0, empty, dra[:5], mask=to_dev(mz), combine="and"))
    assert np.array_equal(got, want_mask(za, za, "!=", False, "and", mz)), (ty, policy, "uniform width 0")
    got = got_mask(fl.FoR.unfor_compare_columns(0, empty, dra[:5], ">", 0, empty, drb[:5], n_blocks=5))
    assert np.array_equal(got, want_mask(za, zb, ">", False)), (ty, policy, "uniform width 0, new")


def test_chain_columns_and_between_then_aggregate(fl):
    """WHERE ship < receipt AND ts BETWEEN a AND b, then COUNT / SUM / MIN / MAX of z: four columns through the library's own encoder
    (block_min_max -> for_widths -> widths_to_offsets -> for_pack_widths), the column predicate chained in place through the range
    predicate's mask, against numpy."""
    import torch
    n = 96
    rng = np.random.default_rng(12300)
    ts = (np.arange(n * 1024, dtype=np.uint64) * 37 + 1000).astype(np.uint32)                # ascending: most blocks decided by BETWEEN
    ship = (20000 + np.arange(n * 1024) // 64 + rng.integers(0, 30, size=n * 1024)).astype(np.uint32)
    receipt = (ship.astype(np.int64) + rng.integers(-3, 12, size=n * 1024)).astype(np.uint32)
    receipt[20 * 1024:21 * 1024] = ship[20 * 1024:21 * 1024].max() + 1                        # blocks the column predicate decides
    receipt[22 * 1024:23 * 1024] = ship[22 * 1024:23 * 1024].min()
    z = rng.integers(0, 50000, size=n * 1024).astype(np.uint16)
    cols = {}
    for name, ty, v in (("ts", "u32", ts), ("ship", "u32", ship), ("receipt", "u32", receipt), ("z", "u16", z)):
        dv = to_dev(v)
        mins, maxs = fl.BitPacking.block_min_max(dv)
        dw = fl.for_widths(mins, maxs)
        doff, dtotal = fl.widths_to_offsets(ty, dw)
        dpk = torch.zeros(max(int(dtotal.item()) // (tbits(ty) // 8), 1), dtype=getattr(torch, TDT[ty]), device="cuda:0")
        fl.for_pack_widths(dw, doff, dv, mins, dpk)
        cols[name] = (dw, doff, dpk, mins)
    a, b = int(ts[15 * 1024 + 300]), int(ts[33 * 1024 + 77])
    m = fl.unfor_compare_range_widths(*cols["ts"], a, b)
    out = fl.unfor_compare_columns_widths(*cols["ship"], "<", *cols["receipt"], mask=m, combine="and", output=m)
    assert out is m
    keep = (ship < receipt) & (ts >= a) & (ts <= b)
    assert np.array_equal(got_mask(m), np.packbits(keep, bitorder="little").view(np.int32))
    result, _ = fl.unfor_aggregate_widths(*cols["z"], mask=m)
    kept = z[keep].astype(np.uint64)
    assert kept.size > 2048 and not keep[20 * 1024:24 * 1024].all() and keep[20 * 1024:21 * 1024].all() and not keep[22 * 1024:23 * 1024].any()
    assert [int(x) for x in result.cpu().numpy().view(np.uint64)] == [kept.size, int(kept.sum()), int(kept.min()), int(kept.max())]
