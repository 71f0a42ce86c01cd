"""GPU: the kernels that take a minimum or a maximum -- block_min_max, unfor_aggregate, unfor_aggregate_widths, aggregate_reduce,
for_widths -- on columns in which ONE element decides (tests/extrema_data.py): every position of a block holds the strict minimum of
one block and the strict maximum of another, the runner-ups are min + 1 and max - 1 and sit next to their extreme, pair blocks set
the two apart by one chosen bit, and one of the three references makes the values wrap inside every block.  Uniform random data holds
a narrow block's extremes many times over and sets a wide block's extremes apart in their top bits, so a kernel that skipped an element,
let a masked-off row take part or compared wrongly in the low bits would pass the older tests (tests/checker/make_badextrema_sources.py
holds four such defects, the first four of its ten; profiles/extrema_known_bad.txt).

Every expected value is a numpy reduction of the constructed values, or int.bit_length; the columns are packed by the oracle's
for_pack and nothing is unpacked on the host.  Bit-exact.  The coverage conditions are asserted on the CPU before any launch."""
import numpy as np
import pytest

import extrema_data as ed
from oracle_lib import TYPES, tbits
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import IDENTITY, POLICIES, TYS, check_slots, combine, expected_blocks, mask_words, place, sentinel_slots, to_dev, to_np, u64_of

pytestmark = pytest.mark.gpu

U = np.uint64


@pytest.fixture
def column(oracle):
    """column(ty, W, kind) -> (extrema_data.Column, the column packed by the oracle's for_pack): coverage asserted first, each column
    built once and kept until the test releases it (column.clear()) or ends."""
    built = {}

    def get(ty, W, kind):
        key = (ty, W, kind)
        if key not in built:
            T = tbits(ty)
            dt = TYPES[ty][0]
            c = ed.column(T, W, kind)
            ed.check_column(c, kind)
            built[key] = (c, oracle.batch("for_pack", ty, W, c.values.astype(dt), aux=np.full(c.n, c.r, dtype=dt)))
        return built[key]
    get.clear = built.clear
    yield get
    built.clear()


# ---------------------------------------------------------------------------------------------------------------------------------
# block_min_max
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYS)
def test_block_min_max_every_position_decides(fl, column, ty):
    """The sweep blocks' decoded values under the wrapping reference, W in {1, 2, T / 2 + 1, T}: 1024 blocks (W = 1: 2048), each position
    the only minimum of one block and the only maximum of another."""
    T = tbits(ty)
    dt = TYPES[ty][0]
    for W in (1, 2, T // 2 + 1, T):
        c, _ = column(ty, W, "wrap")
        n = c.n_sweep
        v = c.values[:n * 1024].astype(dt)
        mins, maxs = fl.BitPacking.block_min_max(to_dev(v))
        vb = v.reshape(n, 1024)
        for name, got, want, pos in (("min", to_np(mins, ty), vb.min(axis=1), c.min_pos), ("max", to_np(maxs, ty), vb.max(axis=1), c.max_pos)):
            assert got.shape == want.shape
            if not np.array_equal(got, want):
                wrong = np.flatnonzero(got != want)
                b = int(wrong[0])
                raise AssertionError(f"{ty} block_min_max W={W}: {wrong.size} blocks' {name} differ, the first is block {b}: {int(got[b])}, not "
                                     f"{int(want[b])}, which sits at {place(T, pos[b])}")
        column.clear()


# ---------------------------------------------------------------------------------------------------------------------------------
# unfor_aggregate, uniform width
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which_width", range(6))
@pytest.mark.parametrize("ty", TYS)
def test_unfor_aggregate_where_one_element_decides(fl, column, kernel_policy, ty, which_width):
    """W in {1, 2, 3, T / 2 + 1, T - 1, T}, the three references (broadcast), every named mask, the kernel policies of
    test_gpu_aggregate.py (the u8 / u16 static 2- and 4-blocks-per-wavefront shapes and the block-by-block path).  Under `without min`
    the expected minimum of a sweep block is min + 1: a masked-off row that still took part would win."""
    T = tbits(ty)
    W = ed.widths_of(T)[which_width]
    calls = []
    for kind in ed.REFERENCES:
        c, pk = column(ty, W, kind)
        dpk = to_dev(pk)
        for name, bits in c.masks().items():
            calls.append((c, dpk, kind, name, None if bits is None else mask_words(bits), expected_blocks(c.values, bits)))
    for policy in POLICIES:
        kernel_policy(policy)
        for c, dpk, kind, name, dm, want in calls:
            buf, slots = sentinel_slots(c.n)
            result, _ = fl.FoR.unfor_aggregate(W, dpk, c.r, dm, n_blocks=c.n, block_aggs=slots)
            check_slots(buf, c.n, result, want, T, c.min_pos, c.max_pos, f"{ty} unfor_aggregate W={W} reference {kind} ({c.r}) mask '{name}' policy={policy}")
    column.clear()


# ---------------------------------------------------------------------------------------------------------------------------------
# unfor_aggregate_widths, mixed width
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", TYS)
def test_unfor_aggregate_widths_where_one_element_decides(fl, oracle, kernel_policy, ty):
    """One column of 1024 + T blocks, block b of width 1 + b mod T with the sweep pattern of position b mod 1024 and a reference of its
    own (zero, inside the type, wrapping: in turn), then width-0 blocks round one more decoded block -- the constant route next to the
    decode inside one wavefront's group.  The masks and policies of the uniform-width test."""
    import torch
    T = tbits(ty)
    dt = TYPES[ty][0]
    widths, refs, values, min_pos, max_pos, pos = ed.mixed_column(T)
    ed.check_mixed_coverage(T, widths, refs, values, pos)
    n = widths.size
    v = values.astype(dt).reshape(n, 1024)
    r = refs.astype(dt)
    col = np.concatenate([oracle.for_pack(ty, int(w), v[b], r[b]) for b, w in enumerate(widths)])
    off = np.concatenate([[0], np.cumsum(widths.astype(np.int64) * 128)])
    assert off[-1] == col.size * (T // 8)
    dw, doff, dcol, drefs = torch.from_numpy(widths).cuda(), torch.from_numpy(off[:-1].copy()).cuda(), to_dev(col), to_dev(r)
    calls = [(name, None if bits is None else mask_words(bits), expected_blocks(values, bits))
             for name, bits in ed.named_masks(n, min_pos, max_pos, 98100 + T).items()]
    for policy in POLICIES:
        kernel_policy(policy)
        for name, dm, want in calls:
            buf, slots = sentinel_slots(n)
            result, _ = fl.unfor_aggregate_widths(dw, doff, dcol, drefs, dm, block_aggs=slots)
            check_slots(buf, n, result, want, T, min_pos, max_pos, f"{ty} unfor_aggregate_widths mask '{name}' policy={policy}",
                        lambda b: f" (W={int(widths[b])}, reference {int(refs[b])})")


# ---------------------------------------------------------------------------------------------------------------------------------
# aggregate_reduce
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4097, 8193])
def test_aggregate_reduce_finds_the_one_slot_that_is_not_the_identity(fl, n):
    """n identity slots but one, at index 0, 4095, 4096 (the edges of the 4096-slot chunks) or n - 1; its minimum 2^64 - 2 and its
    maximum 1 are next to the identity's 2^64 - 1 and 0."""
    for at in (0, 4095, 4096, n - 1):
        slots = np.tile(IDENTITY, (n, 1))
        slots[at] = np.array([1, 12345, 2 ** 64 - 2, 1], dtype=U)
        want = combine(slots)
        assert [int(x) for x in want] == [1, 12345, 2 ** 64 - 2, 1]
        got = u64_of(fl.aggregate_reduce(to_dev(slots.view(np.int64).reshape(-1)).view(n, 4)))
        assert np.array_equal(got, want), (n, f"the slot at {at}", [int(x) for x in got])


# ---------------------------------------------------------------------------------------------------------------------------------
# for_widths
# ---------------------------------------------------------------------------------------------------------------------------------
def spans_of(T):
    return sorted({0, 1, (1 << T) - 1} | {(1 << k) + d for k in range(1, T) for d in (-1, 0, 1)})


def span_cases(T):
    """(span, min, does min + span stay inside the type) for every span and the four minimums"""
    M = (1 << T) - 1
    seeded = int.from_bytes(np.random.default_rng(98200 + T).bytes(8), "little") & M
    return [(s, m, m + s <= M) for s in spans_of(T) for m in sorted({0, seeded, M - s, M})]


@pytest.mark.parametrize("ty", TYS)
def test_for_widths_at_every_power_of_two(fl, ty):
    """Spans 0, 1, 2^T - 1 and 2^k - 1, 2^k, 2^k + 1 for every k, each above the minimums 0, a seeded one, 2^T - 1 - span and 2^T - 1 (where
    min + span wraps): the bit length of the span."""
    T = tbits(ty)
    dt = TYPES[ty][0]
    M = (1 << T) - 1
    cases = span_cases(T)
    assert any(not inside for _, _, inside in cases) and {1 << k for k in range(1, T)} <= {s for s, _, _ in cases}
    mins = np.array([m for _, m, _ in cases], dtype=U).astype(dt)
    maxs = np.array([(m + s) & M for s, m, _ in cases], dtype=U).astype(dt)
    want = np.array([s.bit_length() for s, _, _ in cases], dtype=np.uint8)
    got = fl.for_widths(to_dev(mins), to_dev(maxs)).cpu().numpy()
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{ty} for_widths: {int((got != want).sum())} widths differ, the first for span {cases[i][0]} above the minimum {cases[i][1]}: "
                             f"{int(got[i])} bits, not {int(want[i])}")


@pytest.mark.parametrize("ty", TYS)
def test_encoder_chain_is_lossless_at_every_power_of_two(fl, ty):
    """The same spans end to end: one block per (span, minimum) holding exactly {min, min + span}, through block_min_max -> for_widths ->
    widths_to_offsets -> for_pack_widths -> unfor_pack_widths.  A span of exactly 2^k needs k + 1 bits."""
    import torch
    T = tbits(ty)
    dt = TYPES[ty][0]
    M = (1 << T) - 1
    cases = span_cases(T)
    n = len(cases)
    rng = np.random.default_rng(98300 + T)
    lo = np.array([m for _, m, _ in cases], dtype=U)[:, None]
    hi = np.array([(m + s) & M for s, m, _ in cases], dtype=U)[:, None]
    v = np.where(rng.random((n, 1024)) < 0.5, lo, hi)
    at = rng.integers(0, 512, size=(n, 2))
    v[np.arange(n), at[:, 0]] = lo[:, 0]
    v[np.arange(n), 512 + at[:, 1]] = hi[:, 0]
    want_min, want_max = v.min(axis=1), v.max(axis=1)
    want_w = np.array([int(int(b) - int(a)).bit_length() for a, b in zip(want_min, want_max)], dtype=np.uint8)
    for i, (s, _, inside) in enumerate(cases):
        assert not inside or int(want_w[i]) == s.bit_length()
    v = v.astype(dt).reshape(-1)
    dv = to_dev(v)
    mins, maxs = fl.BitPacking.block_min_max(dv)
    assert np.array_equal(to_np(mins, ty), want_min.astype(dt)) and np.array_equal(to_np(maxs, ty), want_max.astype(dt)), (ty, "block_min_max")
    dw = fl.for_widths(mins, maxs)
    got_w = dw.cpu().numpy()
    if not np.array_equal(got_w, want_w):
        i = int(np.flatnonzero(got_w != want_w)[0])
        raise AssertionError(f"{ty} for_widths in the encoder chain: block {i} holds {int(want_min[i])} and {int(want_max[i])} (span {int(want_max[i]) - int(want_min[i])}) "
                             f"and gets {int(got_w[i])} bits, not {int(want_w[i])}")
    doff, dtotal = fl.widths_to_offsets(ty, dw)
    assert int(dtotal.item()) == int(want_w.astype(np.int64).sum()) * 128
    dpk = torch.zeros(int(dtotal.item()) // (T // 8), dtype=dv.dtype, device="cuda:0")
    fl.for_pack_widths(dw, doff, dv, mins, dpk)
    back = to_np(fl.unfor_pack_widths(dw, doff, dpk, mins), ty)
    if not np.array_equal(back, v):
        b = int(np.flatnonzero(back != v)[0]) // 1024
        raise AssertionError(f"{ty}: the encoder chain loses block {b}, which holds {int(want_min[b])} and {int(want_max[b])} at {int(want_w[b])} bits")
