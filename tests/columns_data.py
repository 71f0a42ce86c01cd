"""What the tests of unfor_compare_columns share (numpy and Python integers only, no GPU): the decision rule restated over big
integers, the expected mask, and the recipe of the column pairs the GPU test runs."""
import numpy as np

OPS = ["==", "!=", "<", "<=", ">", ">="]            # fl_cmp 0..5
MIRROR = {"==": "==", "!=": "!=", "<": ">", "<=": ">=", ">": "<", ">=": "<="}     # a <op> b  ==  b <MIRROR[op]> a
EACH, ALL, NONE = 0, 1, 2
PY = {"==": lambda a, b: a == b, "!=": lambda a, b: a != b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b,
      ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}
SIGNED_VIEW = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def hull(T, r, w):
    """[lo, hi] of the cyclic range [r, r + 2^w - 1] mod 2^T: a range that wraps holds both 0 and M"""
    N = 1 << T
    span = (1 << w) - 1
    return (0, N - 1) if r + span >= N else (r, r + span)


def columns_verdict(T, op, signed, ra, wa, rb, wb):
    """The rule of fl_columns_decide.hpp as the issue of unfor_compare_columns states it, op by op, over Python integers: the verdict of
    `a <op> b` for blocks with raw references ra / rb and widths wa / wb."""
    N = 1 << T
    bias = N >> 1 if signed else 0
    ra, rb = (ra + bias) % N, (rb + bias) % N
    if op in ("==", "!="):
        disjoint = (rb - ra) % N > (1 << wa) - 1 and (ra - rb) % N > (1 << wb) - 1
        same = wa == 0 and wb == 0 and ra == rb
        if op == "==":
            return NONE if disjoint else ALL if same else EACH
        return ALL if disjoint else NONE if same else EACH
    (lo_a, hi_a), (lo_b, hi_b) = hull(T, ra, wa), hull(T, rb, wb)
    if op in (">", ">="):                                                   # the mirror of < / <=
        (lo_a, hi_a), (lo_b, hi_b) = (lo_b, hi_b), (lo_a, hi_a)
    if op in ("<", ">"):
        return ALL if hi_a < lo_b else NONE if lo_a >= hi_b else EACH
    return ALL if hi_a <= lo_b else NONE if lo_a > hi_b else EACH


def hit_bits(va, vb, op, signed):
    """the definition on the decoded values: one bool per row; signed: on the signed view of the dtype"""
    if signed:
        view = SIGNED_VIEW[va.dtype.itemsize]
        va, vb = va.view(view), vb.view(view)
    return PY[op](va, vb)


def want_mask(va, vb, op, signed, combine="new", mask_in=None):
    """32 int32 words per 1024-value block, bit i of word i // 32, LSB first"""
    hit = np.packbits(hit_bits(va, vb, op, signed), bitorder="little").view(np.int32)
    return hit if combine == "new" else (mask_in & hit) if combine == "and" else (mask_in | hit)


def pair_references(T, widths_a, widths_b, seed, dtype):
    """References of a column pair: r_a random; r_b = r_a + d with d drawn inside (-2^WB, 2^WA), so that the two ranges overlap --
    except every block with b % 4 == 1 (d = 2^WA: a < b everywhere) and b % 4 == 3 (d = -2^WB: a > b everywhere)."""
    rng = np.random.default_rng(seed)
    N = 1 << T
    ra, rb = [], []
    for b, (wa, wb) in enumerate(zip(widths_a, widths_b)):
        wa, wb = int(wa), int(wb)
        r = int(rng.integers(0, N - 1, dtype=np.uint64, endpoint=True))
        if b % 4 == 1:
            d = 1 << wa
        elif b % 4 == 3:
            d = -(1 << wb)
        else:
            d = int(rng.integers(-(1 << wb) + 1, (1 << wa) - 1, endpoint=True)) if max(wa, wb) < 63 else \
                int(rng.integers(0, (1 << wa) - 1, dtype=np.uint64, endpoint=True)) - int(rng.integers(0, (1 << wb) - 1, dtype=np.uint64, endpoint=True))
        ra.append(r)
        rb.append((r + d) % N)
    return np.array(ra, dtype=np.uint64).astype(dtype), np.array(rb, dtype=np.uint64).astype(dtype)


# single-bit positions: the block's ends, the ends of the 16-byte slices lanes 0..7 load and store, and the first and last index of a
# lane's cell (16 / 8 / 4 / 2 indices for u8 / u16 / u32 / u64) in the first and a later 1-KiB group
ONE_BIT = [0, 1023, 127, 128, 895, 896] + [base + 5 * n + e for n in (16, 8, 4, 2) for base in (0, 512) for e in (0, n - 1)]


def incoming_mask(n, seed, shift=0):
    """[n * 32] int32: random half-density blocks mixed with all-zero blocks, all-ones blocks, blocks with ONE bit set and blocks with
    one bit clear; `shift` rotates which block gets which kind"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << 32, size=(n, 32), dtype=np.uint64).astype(np.uint32)
    for b in range(n):
        kind = (b + shift) % 6
        if kind == 1:
            m[b] = 0
        elif kind == 2:
            m[b] = 0xFFFFFFFF
        elif kind in (4, 5):
            i = ONE_BIT[((b + shift) // 6) % len(ONE_BIT)]
            m[b] = 0
            m[b, i // 32] = np.uint32(1) << np.uint32(i % 32)
            if kind == 5:
                m[b] = ~m[b]
    return m.reshape(-1).view(np.int32)
