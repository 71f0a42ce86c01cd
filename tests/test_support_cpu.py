"""CPU: the expected-value side of the GPU tests (tests/gpu_support.py: the mask set, the mixed-width column's layout, numpy's
comparison mask, the per-block aggregates and their combination) gives what it gave when every test file kept its own copy.  The
literals below were recorded at d77c18f from that commit's copies -- test_gpu_select.mask_set and test_gpu_aggregate.mask_set,
the four mixed_column (torch.from_numpy(...).cuda() replaced by a stand-in that hands the numpy array back), both want_mask,
test_gpu_aggregate.expected_blocks and combine -- and never from gpu_support itself: a change to a seed's masks, to a column's
bytes or to a reference value fails here, without a GPU, torch or the built library."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_support as gs
from oracle_lib import TYPES, packed_len, tbits


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# mask_set(5, np.random.default_rng(14100 + 32)): name -> (popcount, SHA-256 of np.packbits(bits, bitorder="little")), in order
MASKS = [
    ("zeros", (0, "9e132485d5107211de325a45e7917cbe3e4b5b9cde3e4ee91d7d2102317759ee")),
    ("ones", (5120, "19ec806316e644d8865311c13826f0e5ffe27b39af49471137b3fbae4103b44b")),
    ("bit 0", (5, "501d5176799d81addb3416e6cc73756e292a4500f51d3b460ab01d07fbcbe94c")),
    ("bit 31", (5, "fed20ddd96e4c621b7cde1d19ef662d350a8cb8075d827b90e6f89981b3bfda9")),
    ("bit 32", (5, "2f4512e97b323f66dd011139f95ea26594500a442d12da6d76a4c3601950db19")),
    ("bit 1022", (5, "ba8d9f25971fc67ade8aa4bb27dd9e8f47e0fcabf1f82cc73197f3e96e64187c")),
    ("bit 1023", (5, "93839c80104a74ca9385649e26e3f95e99f54c5746e0753427b12bbf9c12ec9b")),
    ("0xAAAAAAAA", (2560, "7f6e495c2d385dc56a4a9fd33063b160d71d3d72e8dde31d3481e475f118d895")),
    ("random 1/1024", (5, "5d73023d814660f75ea681160b8e7f6034346052c13b6ed80e98f8fee8729363")),
    ("random 1 %", (53, "2958c3c17d9a50409081f3930cf8c1e1385df88778f7542f2363736c3ac130e6")),
    ("random 50 %", (2553, "21a89aef141a43238bbb4e469bcfaf3cdfe5fba2b02d15f214fad83f99c3b376")),
    ("alternate", (2048, "7fa159ec3bf61775342e157a41869bcb2e64206305b03f1d9d3e4502b7959290")),
    ("last block only", (305, "95a0fd6c9db4ad47e4f33f13756c0ed6d7cc790b3992f6e75c372dd0befc97e7")),
]
# full=False keeps these; the densities and the last block are drawn as for the full set, so the masks kept are the same masks
SHORT = ("zeros", "ones", "bit 1023", "0xAAAAAAAA", "random 1 %", "random 50 %", "alternate", "last block only")


def recorded(masks):
    return [(k, None if v is None else (int(v.sum()), sha(np.packbits(v, bitorder="little")))) for k, v in masks.items()]


def test_mask_set_is_the_set_of_the_select_and_aggregate_tests():
    def rng():
        return np.random.default_rng(14100 + 32)
    short = [m for m in MASKS if m[0] in SHORT]
    assert [m[0] for m in short] == list(SHORT)
    # test_gpu_select.mask_set
    assert recorded(gs.mask_set(5, rng())) == MASKS and recorded(gs.mask_set(5, rng(), True)) == MASKS
    assert recorded(gs.mask_set(5, rng(), full=False)) == short
    # test_gpu_aggregate.mask_set: the same, then "no mask"
    assert recorded(gs.mask_set(5, rng(), with_none=True)) == MASKS + [("no mask", None)]
    assert recorded(gs.mask_set(5, rng(), full=False, with_none=True)) == short + [("no mask", None)]
    for bits in gs.mask_set(5, rng()).values():
        assert bits.dtype == bool and bits.shape == (5 * 1024,)


def test_mixed_column_layout():
    """mixed_column("u16", np.arange(17), seed=7) of all four copies (they agreed): widths, byte offsets, column, per-block slices"""
    widths, off, col, blocks = gs.mixed_column_host("u16", np.arange(17), 7)
    assert widths.dtype == np.uint8 and widths.tolist() == list(range(17))
    assert off.dtype == np.int64
    assert off.tolist() == [0, 0, 128, 384, 768, 1280, 1920, 2688, 3584, 4608, 5760, 7040, 8448, 9984, 11648, 13440, 15360]
    assert col.dtype == np.uint16 and col.size == 8704
    assert sha(col) == "60143d3309746c3b820df13c6e8ab43ccb7f11720c382f8c712d11aec0e82224"
    assert [(w, len(pk)) for w, pk in blocks] == [(w, 64 * w) for w in range(17)]
    assert all(type(w) is int for w, _ in blocks)
    assert sha(np.concatenate([pk for _, pk in blocks])) == sha(col)            # the slices tile the column, in order
    # a list of widths, as the range tests pass it
    w2, off2, col2, _ = gs.mixed_column_host("u16", list(range(17)), 7)
    assert w2.dtype == np.uint8 and np.array_equal(off2, off) and np.array_equal(col2, col)


def two_blocks():
    """one fixed 2-block u32 array, a half-density mask over it, and a constant that occurs in it"""
    r = np.random.default_rng(20260)
    vals = r.integers(0, 1 << 32, size=2048, dtype=np.uint64).astype(np.uint32)
    bits = r.random(2048) < 0.5
    assert sha(vals) == "7a221dd102012ee0484e384f6fb8a6343f346d9abf2de07db7482b55ae73a5b3"
    assert sha(np.packbits(bits, bitorder="little")) == "5b57192ed7b1cbdfa3b03cd8a62ce98531f8236910b53a469b0e7d13193202a7"
    assert int(vals[100]) == 3366719290
    return vals, bits, 3366719290


def test_want_mask_of_the_six_ops():
    """test_gpu_for_compare.want_mask and test_gpu_compare_boundaries.want_mask (they agreed): op -> (set bits, SHA-256 of the words)"""
    vals, _, k = two_blocks()
    want = {"==": (1, "6fc8f91ef81c360b092632e0f924a4679213c2152948f2070d1ce5395782ea94"),
            "!=": (2047, "8befee42893d0a4e68bd19087eb3650791bab46ed818e9830d67e4141391e2fd"),
            "<": (1623, "d75ea168949623593b421f7e13b69c82e4df1308d653d93c1872213bed8d131d"),
            "<=": (1624, "4ee57c3b2bd977cd69d62722916d0cc8d325a60db7f7f4003c405a1b6046ce15"),
            ">": (424, "35e83a6fc9954dba61082a4f63559aa3d7c59acfcf53ec222c8e689b75684d6b"),
            ">=": (425, "f822ce2efad6490b95b49db5e54e2f9f4921096134b79fdb9e4d954a2fbc5e06")}
    assert list(gs.CMP) == list(want)
    for op, (count, digest) in want.items():
        m = gs.want_mask(vals, op, k)
        assert m.dtype == np.int32 and m.shape == (64,)
        assert (int(np.unpackbits(m.view(np.uint8)).sum()), sha(m)) == (count, digest), op


def test_expected_blocks_and_combine():
    """test_gpu_aggregate.expected_blocks / combine: count, wrapping sum, min, max per block and over the column"""
    vals, bits, _ = two_blocks()
    for b, blocks, total in (
            (bits, [[545, 1180502940127, 8285431, 4284814077], [523, 1133089519718, 17776666, 4293140581]],
             [1068, 2313592459845, 8285431, 4293140581]),
            (None, [[1024, 2208444685164, 1395954, 4284814077], [1024, 2203538432670, 17776666, 4293140581]],
             [2048, 4411983117834, 1395954, 4293140581])):
        e = gs.expected_blocks(vals, b)
        assert e.dtype == np.uint64 and e.tolist() == blocks
        c = gs.combine(e)
        assert c.dtype == np.uint64 and c.tolist() == total
    empty = gs.combine(np.zeros((0, 4), np.uint64))
    assert empty.tolist() == [0, 0, 18446744073709551615, 0] == gs.IDENTITY.tolist()
    empty[0] = 1
    assert gs.IDENTITY[0] == 0                                                  # a copy: the shared constant stays as it is


def test_constants():
    assert gs.TYS == ["u8", "u16", "u32", "u64"] and gs.GUARD == 96
    assert gs.TDT == {"u8": "uint8", "u16": "uint16", "u32": "uint32", "u64": "uint64"}
    assert gs.SIGNED == {"u8": "uint8", "u16": "int16", "u32": "int32", "u64": "int64"}
    assert gs.POLICIES == [0, 1, 2, 17040386, 198146]
    assert int(gs.SENTINEL) == 0xA5A5A5A5A5A5A5A5
    assert [int(gs.sentinel_of(ty)) for ty in gs.TYS] == [0xA5, 0xA5A5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5]
    assert [gs.sentinel_of(ty).dtype.itemsize for ty in gs.TYS] == [1, 2, 4, 8]


# ---- the conditions tests/test_gpu_alignment.py rests on: its columns reach every 16-byte residue, and a kernel that rounded an
# address to 128 bytes would decode something else (so those tests can fail) ----
def decode_at(oracle, ty, w, image, pos):
    """the oracle's unpack of the 128 * w bytes at byte `pos` of `image` (uint8)"""
    return oracle.unpack(ty, w, image[pos:pos + 128 * w].copy().view(TYPES[ty][0]))


@pytest.mark.parametrize("n", gs.ALIGNED_COLUMN_BLOCKS)
@pytest.mark.parametrize("ty", gs.TYS)
def test_aligned_columns_reach_every_residue_and_every_route(ty, n):
    T = tbits(ty)
    widths, off, col, blocks, gaps = gs.aligned_column_host(ty, n)
    spec_w, pad16, _ = gs.aligned_column_spec(ty, n)
    assert widths.size == n == off.size == len(blocks) and np.array_equal(widths, spec_w) and widths.max() <= T
    assert (off % 16 == 0).all() and off.dtype == np.int64
    size = widths.astype(np.int64) * 128
    assert off[0] == 16 * pad16[0] and (off[1:] == off[:-1] + size[:-1] + 16 * pad16[1:]).all()       # in order, no overlap
    assert off[-1] + size[-1] == col.nbytes
    assert set((off % 128).tolist()) == set(range(0, 128, 16))
    if n > T:
        assert widths[:T + 1].tolist() == list(range(T + 1))
    assert {0, T, T // 2 - 1, T // 2} <= set(widths.tolist())
    assert 2 * (T // 2 - 1) < T <= 2 * (T // 2)
    # the byte map: exactly the bytes no block covers, and the blocks are the column's bytes at their offsets
    assert gaps.dtype == bool and gaps.shape == (col.nbytes,) and int(gaps.sum()) == 16 * int(pad16.sum())
    raw = col.view(np.uint8)
    for (w, pk), o in zip(blocks, off):
        assert w * 128 == pk.nbytes and not gaps[o:o + pk.nbytes].any() and np.array_equal(pk.view(np.uint8), raw[o:o + pk.nbytes])
    # wherever the column's base lies, blocks that hold bytes start on all eight residues
    for base in gs.ALIGNED_COLUMN_BASES:
        assert set(((off + base) % 128)[widths > 0].tolist()) == set(range(0, 128, 16)), base


@pytest.mark.parametrize("n", gs.ALIGNED_COLUMN_BLOCKS)
@pytest.mark.parametrize("ty", gs.TYS)
def test_aligned_columns_decode_differently_from_a_rounded_offset(oracle, ty, n):
    """offsets[b] rounded down or up to 128 -- inside the column, and as an address with the column at its two residues -- gives
    another block than offsets[b] does, for every block that does not start on a 128-byte boundary"""
    widths, off, col, blocks, _ = gs.aligned_column_host(ty, n)
    raw = col.view(np.uint8)
    want = [oracle.unpack(ty, w, pk) for w, pk in blocks]
    checked = 0
    for b, (w, o) in enumerate(zip(widths.tolist(), off.tolist())):
        if w == 0 or o % 128 == 0:
            continue
        assert np.array_equal(decode_at(oracle, ty, w, raw, o), want[b])
        for pos in (o - o % 128, o - o % 128 + 128):
            if pos + 128 * w <= raw.size:
                assert not np.array_equal(decode_at(oracle, ty, w, raw, pos), want[b]), (b, w, o, pos)
                checked += 1
    assert checked >= n
    for base in gs.ALIGNED_COLUMN_BASES:
        image, start = gs.placed_image(col, base, gs.column_seed(ty, n, base))
        assert start % 128 == base and np.array_equal(image[start:start + raw.size], raw)
        for b, (w, o) in enumerate(zip(widths.tolist(), off.tolist())):
            at = start + o
            if w == 0 or at % 128 == 0:
                continue
            for pos in (at - at % 128, at - at % 128 + 128):
                assert pos + 128 * w <= image.size
                assert not np.array_equal(decode_at(oracle, ty, w, image, pos), want[b]), (base, b, w, o, pos)


@pytest.mark.parametrize("ty", gs.TYS)
def test_placed_uniform_columns_decode_differently_from_a_rounded_base(oracle, ty):
    """the uniform-width inputs of the alignment tests, with the guard bytes their allocation holds in front of and behind them:
    every block decoded from the base rounded down or up to 128 differs from the block itself"""
    T = tbits(ty)
    n = gs.UNIFORM_BLOCKS
    for w in gs.uniform_widths(ty) + [T // 2 + 1]:
        if w == 0:
            continue
        pk = gs.uniform_packed(ty, w)
        assert pk.size == n * packed_len(ty, w)
        want = oracle.batch("unpack", ty, w, pk).reshape(n, 1024)
        for residue in range(16, 128, 16):
            image, start = gs.placed_image(pk, residue, gs.packed_seed(ty, w, residue))
            assert start % 128 == residue and start >= gs.PLACED_FRONT and image.size - start - pk.nbytes >= gs.PLACED_FRONT
            assert np.array_equal(image[start:start + pk.nbytes], pk.view(np.uint8))
            for base in (start - residue, start - residue + 128):
                for b in (0, 1, n // 2, n - 1):
                    assert not np.array_equal(decode_at(oracle, ty, w, image, base + 128 * w * b), want[b]), (w, residue, base, b)


def test_placed_image_is_seeded_and_keeps_its_guard_under_any_base():
    pay = np.arange(48, dtype=np.uint8)
    a, sa = gs.placed_image(pay, 48, 5)
    b, sb = gs.placed_image(pay, 48, 5, base=0x7f0000000040)
    assert sa == 256 + 48 and (0x7f0000000040 + sb) % 128 == 48 and sb >= gs.PLACED_FRONT
    assert np.array_equal(a[sa - 256:], b[sb - 256:])                          # the same bytes around the payload
    assert np.array_equal(a[sa:sa + 48], pay) and a.size == sa + 48 + gs.PLACED_FRONT
    c, _ = gs.placed_image(pay, 48, 6)
    assert not np.array_equal(a[:sa], c[:sa]) and not np.array_equal(a[sa + 48:], c[sa + 48:])
    assert len(set(a[:sa].tolist())) > 64 and len(set(a[sa + 48:].tolist())) > 64   # neither zeros nor one sentinel
    assert gs.policy_bpw(0) == 4 and [gs.policy_bpw(p) for p in gs.POLICIES] == [4, 1, 4, 4, 3]
    assert gs.ALIGNED_COLUMN_BLOCKS == [10, 28, 37, 109]
    # a slab of arrays whose sizes are multiples of 128 (packed blocks, unpacked blocks, bases): every residue, no overlap
    sizes = [640, 0, 128, 1152, 4224, 256, 8192, 384, 128]
    starts, total = gs.slab_layout(sizes)
    assert starts[0] == 0 and all(s % 16 == 0 for s in starts) and {s % 128 for s in starts[:8]} == set(range(0, 128, 16))
    assert [b - (a + n) for a, n, b in zip(starts, sizes, starts[1:])] == [16 * (i % 8) for i in range(1, 9)]
    assert total == starts[-1] + sizes[-1]


def test_importing_the_support_module_does_not_import_torch():
    """collection, and the tests above, must not need torch; other test modules import it, so a fresh interpreter is asked"""
    code = "import sys; import gpu_support; assert 'torch' not in sys.modules and 'fastlanes_amd' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)))
