"""What the tests of undelta_compare_range share (numpy and the oracle only; no GPU, no torch): the definition's expected mask, the
block decision and route read off the DEFINITION (not off fl_delta_decide.hpp), a numpy model of the kernel's group placement, Delta
columns of random bytes, and SORTED columns encoded on the CPU the way a FastLanes writer encodes them."""
import numpy as np

import bitmodel
from datagen import values
from oracle_lib import TYPES, lanes, tbits

EACH, ALL, NONE, BASES = 0, 1, 2, 3
KEEP, SKIP = "keep", "skip"
COMBINE = ["new", "and", "or"]
FORMS = ("undelta_compare_range", "undelta_compare_range_widths")


def lane_base(l):
    """first ORIGINAL row of FastLanes lane l's chain (fl_device.hpp: lane_base)"""
    return (l % 16) * 64 + bitmodel.FL_ORDER[l // 16] * 8


def hit_bits(vals, lo, hi):
    """the definition, in the values' own unsigned type (numpy wraps mod 2^T): one bool per value"""
    dt = vals.dtype.type
    with np.errstate(over="ignore"):
        return (vals - dt(lo)) <= dt((hi - lo) % (1 << (8 * vals.dtype.itemsize)))


def want_mask(vals, lo, hi, combine="new", mask_in=None):
    """32 int32 words per 1024-value block, bit i of word i // 32, LSB first; i = the ORIGINAL row"""
    hit = np.packbits(hit_bits(vals, lo, hi), bitorder="little").view(np.int32)
    return hit if combine == "new" else (mask_in & hit) if combine == "and" else (mask_in | hit)


def decode(oracle, ty, blocks, bases):
    """untranspose(undelta_pack::<W_b>(block b, bases[b])) of every (w, packed) block: the column in original row order"""
    L = lanes(ty)
    return np.concatenate([oracle.untranspose(ty, oracle.undelta_pack(ty, w, pk, bases[b * L:(b + 1) * L])) for b, (w, pk) in enumerate(blocks)])


def decode_uniform(oracle, ty, w, packed, bases, n):
    return oracle.batch("untranspose", ty, None, oracle.batch("undelta_pack", ty, w, packed, aux=bases, n_blocks=n))


def verdict_of(T, lo, hi, bases, w):
    """The block decision from the definition, in Python's exact integers: lane l's values are base_l plus 1 .. T deltas of [0, 2^W - 1],
    so relative to lo they lie in [c_l, c_l + T (2^W - 1)] before any wrap."""
    N = 1 << T
    s = (hi - lo) % N
    cs = [(int(b) - lo) % N for b in bases]
    reach = T * ((1 << w) - 1)
    if s == N - 1 or all(c + reach <= s for c in cs):
        return ALL
    if all(c > s and c + reach <= N - 1 for c in cs):
        return NONE
    return BASES if w == 0 else EACH


def route_of(T, lo, hi, bases, w, combine, mask_block):
    """KEEP ahead of the decision, as the kernel's routes are ordered"""
    if combine == "and" and not mask_block.any():
        return KEEP
    if combine == "or" and (mask_block == -1).all():
        return KEEP
    return verdict_of(T, lo, hi, bases, w)


def placement_model(ty, w, packed, bases, lo, hi):
    """One block's 32 mask words WITHOUT untransposing a value: every FastLanes lane's chain is summed along its rows (the fields come
    from tests/bitmodel.py's reading of the wire format), each row is judged, and lane l's T verdicts go to bits lane_base(l) ..
    lane_base(l) + T - 1 of the block's 1024-bit mask."""
    T = tbits(ty)
    N = 1 << T
    fields = bitmodel.unpack_bits([int(x) for x in packed], T, w)
    s = (hi - lo) % N
    bits = np.zeros(1024, bool)
    filled = np.zeros(1024, bool)
    for l in range(1024 // T):
        run = int(bases[l])
        for r in range(T):
            run = (run + fields[bitmodel.index(r, l)]) % N
            assert not filled[lane_base(l) + r]
            filled[lane_base(l) + r] = True
            bits[lane_base(l) + r] = ((run - lo) % N) <= s
    assert filled.all()                                                     # the groups tile the mask: nothing placed twice, nothing left out
    return np.packbits(bits, bitorder="little").view(np.int32)


def random_bases(ty, n, seed):
    return values(ty, n * lanes(ty), seed)


def bases_range(T, lo, bases, w):
    """(cmin, cmax, reach) of a block relative to lo, exact integers"""
    N = 1 << T
    cs = [(int(b) - lo) % N for b in bases]
    return min(cs), max(cs), T * ((1 << w) - 1)


def intervals_for(ty, widths, bases, picks):
    """the interval families of the FoR range test: full, wrapping, single-value, and bounds at each side of the picked blocks'
    [min base, max base + T (2^W - 1)]"""
    T = tbits(ty)
    N = 1 << T
    H = N >> 1
    L = lanes(ty)
    out = [(0, N - 1), (5, 4), (N - 1, 0), (1, N - 2), (H, H - 1), (H - 3, H + 3), (H + 3, H - 3), (0, 0), (N - 1, N - 1)]
    for b in picks:
        bb = [int(x) for x in bases[b * L:(b + 1) * L]]
        reach = T * ((1 << int(widths[b])) - 1)
        e = [(min(bb) - 1) % N, min(bb), (max(bb) + reach) % N, (max(bb) + reach + 1) % N]
        out += [(e[1], e[2]), (e[0], e[3]), (e[3], e[0]), (e[2], e[1]), (e[1], e[1]), (e[2], e[2]), (e[0], e[2]), (e[1], e[3])]
    return list(dict.fromkeys(out))


def sorted_column(oracle, ty, n, seed):
    """A nondecreasing column (mod 2^T: the narrow types wrap round) of n blocks, Delta-coded on the CPU: base_l = the original-order
    predecessor of lane l's first row (the column's first value for row 0 of block 0), each block's width from its largest delta.
    Returns (values in original order, widths, (w, packed) per block, bases); the round trip through the oracle is asserted."""
    T = tbits(ty)
    dt = TYPES[ty][0]
    L = lanes(ty)
    rng = np.random.default_rng(seed)
    # per block a step size of its own, so the widths differ; blocks of constant value (width 0) among them
    top = np.array([0 if b % 7 == 3 else (1 << int(rng.integers(0, {8: 1, 16: 4, 32: 10, 64: 20}[T]))) for b in range(n)], dtype=np.uint64)
    steps = (rng.integers(0, 1 << 62, size=(n, 1024), dtype=np.uint64) % (top[:, None] + np.uint64(1))).reshape(-1)
    if T >= 32:
        steps = np.maximum(steps, np.uint64(1)) * np.repeat(top > 0, 1024)  # strictly ascending inside a block with a width
    start = int(rng.integers(0, 1 << (T - 1)))
    with np.errstate(over="ignore"):
        v = (np.cumsum(steps, dtype=np.uint64) + np.uint64(start)).astype(dt)
        prev = np.concatenate([v[:1], v[:-1]])
        d = (v - prev).astype(dt)
    widths, blocks, bases = [], [], np.empty(n * L, dtype=dt)
    for b in range(n):
        vb, db = v[b * 1024:(b + 1) * 1024], d[b * 1024:(b + 1) * 1024]
        for l in range(L):
            bases[b * L + l] = prev[b * 1024 + lane_base(l)]
        w = int(db.max()).bit_length()
        pk = oracle.pack(ty, w, oracle.transpose(ty, db))
        assert np.array_equal(oracle.delta(ty, oracle.transpose(ty, vb), bases[b * L:(b + 1) * L]), oracle.transpose(ty, db)), (ty, b)
        assert np.array_equal(oracle.untranspose(ty, oracle.undelta_pack(ty, w, pk, bases[b * L:(b + 1) * L])), vb), (ty, b, w)
        widths.append(w)
        blocks.append((w, pk))
    return v, np.array(widths, dtype=np.uint8), blocks, bases


def column_of(blocks, ty):
    """(int64 byte offsets, packed column) of (w, packed) blocks laid back to back"""
    esz = tbits(ty) // 8
    sizes = np.array([pk.size * esz for _, pk in blocks], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    col = np.concatenate([pk for _, pk in blocks]) if blocks else np.zeros(0, dtype=TYPES[ty][0])
    return off.astype(np.int64), col


def edge_rows(ty):
    """rows inside a block where ONE element decides: the block's ends, and the first and last row of a T-bit group and of an R = T/8
    row piece, in the first group, a middle one and the last"""
    T = tbits(ty)
    R = T // 8
    rows = {0, 1023}
    for g in (0, T, 5 * T if 5 * T < 1024 else T, 1024 - T):
        rows |= {g, g + T - 1, g + R - 1, g + R, g + T - R - 1, g + T - R}
    return sorted(r for r in rows if 0 <= r < 1024)


def incoming_mask(n, seed, shift=0):
    """[n * 32] int32: random half-density blocks mixed with all-zero blocks, all-ones blocks, blocks with ONE bit set and blocks with
    one bit clear; `shift` rotates which block gets which kind"""
    one_bit = [0, 1023, 127, 128, 895, 896, 31, 32, 63, 64, 7, 8, 519, 520]
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << 32, size=(n, 32), dtype=np.uint64).astype(np.uint32)
    for b in range(n):
        kind = (b + shift) % 6
        if kind == 1:
            m[b] = 0
        elif kind == 2:
            m[b] = 0xFFFFFFFF
        elif kind in (4, 5):
            i = one_bit[((b + shift) // 6) % len(one_bit)]
            m[b] = 0
            m[b, i // 32] = np.uint32(1) << np.uint32(i % 32)
            if kind == 5:
                m[b] = ~m[b]
    return m.reshape(-1).view(np.int32)



def delta_bases(ty, n, seed):
    """LANES bases per block, the kind by b % 4: 0 and 3 random (the chains wrap, nothing decides the block but the full interval), 1
    clustered within 6 of one another, 2 all equal -- blocks the bases can decide when the width is narrow"""
    T = tbits(ty)
    L = lanes(ty)
    dt = TYPES[ty][0]
    rng = np.random.default_rng(seed)
    out = values(ty, n * L, seed + 1).copy()
    for b in range(n):
        if b % 4 in (1, 2):
            b0 = int(out[b * L])
            spread = rng.integers(0, 6, size=L) if b % 4 == 1 else np.zeros(L, dtype=np.int64)
            out[b * L:(b + 1) * L] = np.array([(b0 + int(x)) % (1 << T) for x in spread], dtype=dt)
    return out


def column_verdicts(ty, lo, hi, bases, widths):
    """verdict_of for every block of a column (the lanes' min / max by numpy, in the type's own wrapping arithmetic)"""
    T = tbits(ty)
    N = 1 << T
    dt = TYPES[ty][0]
    with np.errstate(over="ignore"):
        c = (bases - dt(lo)).reshape(-1, lanes(ty))
    s = (hi - lo) % N
    out = []
    for cmin, cmax, w in zip(c.min(axis=1).tolist(), c.max(axis=1).tolist(), widths):
        reach = T * ((1 << int(w)) - 1)
        if s == N - 1 or cmax + reach <= s:
            out.append(ALL)
        elif cmin > s and cmax + reach <= N - 1:
            out.append(NONE)
        else:
            out.append(BASES if int(w) == 0 else EACH)
    return out
