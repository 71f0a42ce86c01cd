"""CPU: the far columns of tests/far_column_data.py are what tests/test_gpu_far_columns.py needs them to be, from the definition and not
from the module's own labels alone: every offset class occurs for every element type, no two blocks or decoys overlap, every offset is
a multiple of 16 inside the buffer, and -- the proof that a kernel which drops offset bits cannot pass -- every far block, read at its
byte addresses mod 2^32 and mod 2^31, is known to the host image and decodes to other values."""
import numpy as np
import pytest

import far_column_data as fcd
from far_column_data import B31, B32, B33, PACKED_BYTES
from oracle_lib import TYPES, load_oracle, tbits

TYS = ["u8", "u16", "u32", "u64"]
CASES = [(ty, v) for ty in TYS for v in fcd.VARIANTS]


def blocks_of(c):
    """(block, width, offset, end) of the blocks that hold bytes"""
    return [(b, int(c.widths[b]), int(c.off[b]), int(c.off[b] + c.sizes[b])) for b in range(c.n) if c.widths[b]]


def test_the_buffer_passes_2_33_and_a_column_is_two_dozen_blocks():
    assert PACKED_BYTES == 2 ** 33 + 2 ** 20 and fcd.N_BLOCKS == 24
    for ty in TYS:
        assert PACKED_BYTES % (tbits(ty) // 8) == 0


@pytest.mark.parametrize("ty,variant", CASES)
def test_every_class_occurs_in_the_primary_column(ty, variant):
    T = tbits(ty)
    c = fcd.far_buffer(ty, variant).columns["a"]
    assert c.n == fcd.N_BLOCKS and c.ty == ty
    held = blocks_of(c)
    offs, ends = {o for _, _, o, _ in held}, {e for _, _, _, e in held}
    assert {0, 1, T // 2, T - 1, T} <= set(c.widths.tolist())
    assert (np.diff(c.off) < 0).any() and (np.diff(c.off) > 0).any(), "offsets must not ascend with the block index"
    # plain
    assert 0 in offs and sum(0 < o and e <= B31 for _, _, o, e in held) >= 1
    # bit 31
    assert B31 in ends and B31 in offs
    # the 2^32 boundary: two of the three in one variant, the third in the other
    straddles = [(o, e) for _, _, o, e in held if o < B32 < e]
    if variant == "edges":
        assert B32 in ends and B32 in offs and not straddles
    else:
        assert len(straddles) == 1 and straddles[0][0] + straddles[0][1] == 2 * B32, "the block's middle lies at 2^32"
    # alias: o + 2^32 with o the offset of another block of the same width below 2^31
    aliases = [(b, w, o) for b, w, o, _ in held if any(o == o2 + B32 and w == w2 and b != b2 and e2 <= B31 for b2, w2, o2, e2 in held)]
    assert aliases and all(c.cls[b] == "alias" for b, _, _ in aliases)
    # bit 33: the byte offset needs bit 33; the element index passes 2^32 for u8 and u16 and reaches 2^31 for u32
    above = [o for _, _, o, _ in held if o >= B33]
    assert above and all(o // (T // 8) >= {8: 2 ** 32, 16: 2 ** 32, 32: 2 ** 31, 64: 2 ** 30}[T] for o in above)
    # width 0 at both ends
    zeros = {int(o) for o, w in zip(c.off, c.widths) if w == 0}
    assert {0, PACKED_BYTES} <= zeros
    # every 16-byte residue mod 128 is a block's start
    assert {o % 128 for o in offs} == set(range(0, 128, 16))


@pytest.mark.parametrize("ty,variant", CASES)
def test_the_labels_say_where_a_block_lies(ty, variant):
    fb = fcd.far_buffer(ty, variant)
    for role, c in fb.columns.items():
        assert c.ty == fcd.column_ty(ty, role) and c.n == fcd.N_BLOCKS
        for b, w, o, e in blocks_of(c):
            k = c.cls[b]
            assert k in fcd.CLASSES and k != "width 0"
            if k == "plain":
                assert e <= B31
            elif k == "bit 31":
                assert B31 - 128 * w <= o <= B32 - 128 * w and e >= B31
            elif k == "2^32":
                assert B32 - 128 * w <= o < B33 and e >= B32
            elif k == "alias":
                assert B32 <= o < B32 + B31 and fb.owner[o - B32][0] == role and fb.owner[o - B32][1] != b
                assert c.widths[fb.owner[o - B32][1]] == w
            else:
                assert o >= B33
        assert all(c.cls[b] == "width 0" for b in range(c.n) if c.widths[b] == 0)
        for k in fcd.FAR_CLASSES:                                               # the other columns take far offsets of every class too
            assert any(c.cls[b] == k for b, _, _, _ in blocks_of(c)), (role, k)
        assert (np.diff(c.off) < 0).any()
        assert np.array_equal(c.compact_off, np.cumsum(c.sizes) - c.sizes) and c.compact.nbytes == c.sizes.sum()


@pytest.mark.parametrize("ty,variant", CASES)
def test_nothing_overlaps_and_every_offset_is_legal(ty, variant):
    fb = fcd.far_buffer(ty, variant)
    spans = sorted((o, o + len(r)) for o, r in fb.regions.items())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two blocks or decoys overlap"
    assert all(o % 16 == 0 and 0 <= o and e <= PACKED_BYTES for o, e in spans)
    n_held = sum(len(blocks_of(c)) for c in fb.columns.values())
    assert len(spans) == n_held + len(fb.decoys) and len(fb.decoys) >= n_held // 3
    for c in fb.columns.values():
        assert (c.off % 16 == 0).all() and (c.off >= 0).all() and (c.off + c.sizes <= PACKED_BYTES).all()
        for b, w, o, e in blocks_of(c):
            assert np.array_equal(fb.read(o, e - o), c.block_bytes(b))
    for s in fb.decoys:                                                         # a decoy is its block complemented, at off mod 2^32 or 2^31
        _, role, b = fb.owner[s]
        c = fb.columns[role]
        assert s in (int(c.off[b]) % B32, int(c.off[b]) % B31) and s != c.off[b]
        assert np.array_equal(fb.regions[s], ~c.block_bytes(b))


@pytest.mark.parametrize("ty,variant", CASES)
def test_a_kernel_that_drops_offset_bits_decodes_other_values(ty, variant):
    """For every block of the bit-31, 2^32, alias and bit-33 classes, of every column, and m = 2^32, 2^31: where any of the block's byte
    addresses changes mod m, the bytes at (off + i) mod m are known to the host image and the oracle decodes them to other values than
    the block's own.  Only a block that ends at or below 2^31 has no address that changes: in the primary column that is the one that
    ends exactly there (its test is the bounds check: off + 128 w as a 32-bit sum is negative as an int and 2^31 as an unsigned)."""
    o = load_oracle()
    fb = fcd.far_buffer(ty, variant)
    for role, c in fb.columns.items():
        dt = TYPES[c.ty][0]
        unmoved = []
        for b, w, off, end in blocks_of(c):
            if c.cls[b] not in fcd.FAR_CLASSES:
                continue
            own = o.unpack(c.ty, w, c.blocks[b][1])
            moved = [m for m in fcd.MODULI if end > m]
            if not moved:
                unmoved.append((off, end))
            for m in moved:
                seen = fb.wrapped_bytes(off, end - off, m)
                assert seen is not None, (role, b, c.cls[b], off, m, "the host image does not know these bytes")
                assert not np.array_equal(seen, c.block_bytes(b))
                assert not np.array_equal(o.unpack(c.ty, w, np.ascontiguousarray(seen).view(dt)), own), (role, b, off, m)
            if off >= B32:
                assert len(moved) == 2
        assert unmoved == ([(B31 - 128 * (tbits(ty) - 1), B31)] if role == "a" else []), (role, unmoved)
