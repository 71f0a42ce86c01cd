"""Columns in which ONE element decides a block's minimum or maximum, for the reducing kernels (block_min_max, unfor_aggregate,
unfor_aggregate_widths, for_widths).

Uniform random data (datagen.values) is nearly blind for an order statistic: a narrow block holds its extremes many times over, so a
kernel that never looked at one row, lane or element would still be right, and the value that should lose a comparison differs from the
winner in its top bits, so a comparison that is wrong in the low bits never changes a result.  The columns made here are built from the
VALUES (the fields are derived from them: field = (value - r) mod 2^T, all below 2^W) and meet, for a type of T bits, a width W >= 1 and
a FoR reference r (check_coverage, asserted on the CPU for every (T, W, r) the GPU tests use):
 1. sweep block b (b = 0..1023) holds its strict minimum at index-order position b and its strict maximum at position 1023 - b; at
    W = 1, where a block cannot hold both, 1024 min-blocks are followed by 1024 max-blocks;
 2. from W = 2 up the second-smallest value of a sweep block is min + 1 and the second-largest max - 1; each occurs at least 8 times
    and sits in the rows above and below and the lanes left and right of its extreme (wrapping round the block's edges) -- except in
    the few blocks (MAX_CROWDED at the most) where the two extremes are so close that such a cell is the other extreme or belongs to
    the minimum's neighbourhood, which goes first;
 3. pair blocks: for each bit j of pair_bits(W) one block whose minimum and runner-up have fields that differ in bit j alone, and one
    block that does the same for the maximum; the extreme sits in an odd lane and the runner-up in the even lane before it (one 16-byte
    cell, one 32-bit word of u8 / u16: whoever walks it meets the runner-up first), and in its other three neighbours;
 4. with the wrapping reference (r = 2^T - 2^(W-1): the fields below 2^(W-1) decode to the top of the type, the others wrap to its
    bottom) every sweep block holds fields of both kinds, its largest value has not wrapped, and its smallest value does not sit at a
    smallest field.

Values and fields are np.uint64 in the unpacked index order (bitmodel.index), [n_blocks * 1024]; nothing here unpacks."""
import numpy as np

from boundary_data import in_index_order

U = np.uint64
REFERENCES = ("zero", "mid", "wrap")
MAX_CROWDED = 16


def seed_of(T, W, kind):
    """The seed of (T, W, reference kind)'s column: the CPU coverage test and the GPU tests build the same arrays."""
    return 99000 + 1000 * REFERENCES.index(kind) + 100 * (T // 8) + W


def reference(T, W, kind):
    """r = 0; a seeded value with r + 2^W - 1 < 2^T where W < T; the wrapping reference 2^T - 2^(W-1)."""
    if kind == "zero":
        return 0
    if kind == "wrap":
        return (1 << T) - (1 << (W - 1))
    rnd = int.from_bytes(np.random.default_rng(seed_of(T, W, kind)).bytes(8), "little")
    return 1 + rnd % ((1 << T) - (1 << W)) if W < T else rnd % (1 << T) | 1


def pair_bits(W):
    return sorted({0, W - 1} | {j for j in (7, 8, 15, 16, 31, 32) if j < W})


def widths_of(T):
    """The widths of the uniform-width GPU tests."""
    return sorted({1, 2, 3, T // 2 + 1, T - 1, T})


def _positions(T):
    """(row, lane) of every index-order position, [1024, 2]"""
    L = 1024 // T
    rl = np.stack(np.meshgrid(np.arange(T), np.arange(L), indexing="ij"), axis=-1).reshape(1, T * L, 2)
    pos = in_index_order(np.arange(T * L, dtype=U).reshape(1, T, L))         # pos[p] = r * L + l
    return rl[0][pos.astype(np.int64)]


def row_lane(T, p):
    r, l = _positions(T)[int(p)]
    return int(r), int(l)


def neighbours(T, dist):
    """[1024, 4] index-order positions `dist` rows above / below and `dist` lanes left / right of each position (wrapping)."""
    L = 1024 // T
    rl = _positions(T)
    at = in_index_order(np.arange(1024, dtype=U).reshape(1, T, L)).astype(np.int64)    # at[p] = r * L + l
    where = np.empty(1024, dtype=np.int64)
    where[at] = np.arange(1024)                                              # where[r * L + l] = p
    r, l = rl[:, 0], rl[:, 1]
    return np.stack([where[((r + dist) % T) * L + l], where[((r - dist) % T) * L + l],
                     where[r * L + (l + dist) % L], where[r * L + (l - dist) % L]], axis=1)


def _available(T, W, r):
    """The decodable values {(f + r) mod 2^T : f < 2^W} as one or two inclusive (lo, hi) intervals of python ints, ascending."""
    S, M = 1 << W, (1 << T) - 1
    if r + S - 1 <= M:
        return [(r, r + S - 1)]
    if S > M:
        return [(0, M)]
    return [(0, r + S - 1 - (M + 1)), (r, M)]


def _sample(rng, T, W, r, lo, hi, size):
    """`size` decodable values in [lo, hi] (python ints), or None when there is none."""
    segs = [(max(a, lo), min(b, hi)) for a, b in _available(T, W, r)]
    segs = [(a, b) for a, b in segs if a <= b]
    if not segs:
        return None
    pick = rng.integers(0, len(segs), size=size)
    raw = np.frombuffer(rng.bytes(8 * size), dtype=U)
    out = np.empty(size, dtype=U)
    for i, (a, b) in enumerate(segs):
        n = b - a + 1
        off = raw if n >> 64 else raw % U(n)
        out[pick == i] = (off + U(a))[pick == i]
    return out


def sweep_blocks(T, W, r, positions, which, rng):
    """[len(positions), 1024] values: block i's strict minimum at positions[i], its strict maximum at 1023 - positions[i] (which = "both",
    W >= 2), or only the one of them (which = "min" / "max", W = 1)."""
    positions = np.asarray(positions, dtype=np.int64)
    n = positions.size
    M = (1 << T) - 1
    S = 1 << W
    avail = _available(T, W, r)
    a_lo, a_hi = avail[0][0], avail[-1][1]
    rows = np.arange(n)
    if W == 1:
        assert which in ("min", "max")
        both = sorted((r & M, (r + 1) & M))
        v = np.full((n, 1024), both[1] if which == "min" else both[0], dtype=U)
        v[rows, positions if which == "min" else 1023 - positions] = both[0] if which == "min" else both[1]
        return v
    assert which == "both"
    wraps = len(avail) == 2
    # how far the extremes may sit inside the decodable range and still leave min + 1 < max - 1 (W = 2: min + 1 = max - 2) decodable
    maxd = min(3, (S // 2 - 2) if wraps else (S - 4) // 2)
    lo = U(a_lo) + (positions % (maxd + 1)).astype(U)
    hi = U(a_hi) - ((positions // 4) % (maxd + 1)).astype(U)
    raw = np.frombuffer(rng.bytes(8 * n * 1024), dtype=U).reshape(n, 1024)
    lo1, hi1 = (lo + U(1))[:, None], (hi - U(1))[:, None]
    if wraps:                                             # [lo + 1, e] and [r, hi - 1]
        e = avail[0][1]
        len1 = (U(e) - lo)[:, None]
        len2 = (hi - U(r))[:, None]
        t = raw % (len1 + len2)
        mid = np.where(t < len1, lo1 + t, U(r) + (t - len1))
    else:                                                 # [lo + 1, hi - 1]
        mid = lo1 + raw % (hi1 - lo1 + U(1))
    choice = rng.integers(0, 4, size=(n, 1024))
    v = np.where(choice == 0, lo1, np.where(choice == 1, hi1, mid))
    pmin, pmax = positions, 1023 - positions
    near, far = neighbours(T, 1), neighbours(T, 2)
    for nb, val in ((far[pmax], hi1), (far[pmin], lo1), (near[pmax], hi1), (near[pmin], lo1)):    # the later ones go first
        v[rows[:, None], nb] = val
    v[rows, pmax] = hi
    v[rows, pmin] = lo
    return v


def pair_block(T, W, r, j, which, rng):
    """1024 values whose minimum (which = "min") or maximum and its runner-up have fields differing in bit j alone; the rest lies beyond
    the runner-up, or on it where nothing beyond is decodable.  Returns (values, position of the extreme)."""
    M = (1 << T) - 1
    FM = (1 << W) - 1
    best = None
    for attempt in range(9):
        fa = (int.from_bytes(rng.bytes(8), "little") & FM & ~(1 << j)) if attempt < 8 else 0
        pair = sorted(((fa + r) & M, ((fa | 1 << j) + r) & M))
        ext, run = pair if which == "min" else pair[::-1]
        rest = _sample(rng, T, W, r, run + 1, M, 1024) if which == "min" else _sample(rng, T, W, r, 0, run - 1, 1024)
        best = (ext, run, rest)
        if rest is not None:
            break
    ext, run, rest = best
    v = np.full(1024, run, dtype=U) if rest is None else rest.copy()
    odd = np.flatnonzero(_positions(T)[:, 1] % 2 == 1)                       # an odd lane: the runner-up in the lane before it shares its cell
    p = int(odd[rng.integers(0, odd.size)])
    v[rng.integers(0, 1024, size=24)] = run
    v[neighbours(T, 1)[p]] = run
    v[p] = ext
    return v, p


class Column:
    """values / fields: np.uint64[n * 1024] in index order; r: the reference; n_sweep: the leading sweep blocks; min_pos / max_pos: per
    block a position that holds the block's minimum / maximum (THE position where it is unique); pairs: (block, bit, "min" / "max")."""

    def __init__(self, T, W, r, values, n_sweep, min_pos, max_pos, pairs):
        self.T, self.W, self.r, self.n_sweep, self.pairs = T, W, r, n_sweep, pairs
        self.values = np.ascontiguousarray(values, dtype=U).reshape(-1)
        self.fields = (self.values - U(r)) & U((1 << T) - 1)
        self.min_pos, self.max_pos = np.asarray(min_pos, dtype=np.int64), np.asarray(max_pos, dtype=np.int64)
        self.n = self.values.size // 1024

    def masks(self):
        return named_masks(self.n, self.min_pos, self.max_pos, seed_of(self.T, self.W, "zero") + 7)


def designated(v):
    """(min_pos, max_pos) of [n, 1024] values: the first position of each block's minimum, and of its maximum (elsewhere if constant)."""
    pmin, pmax = v.argmin(axis=1), v.argmax(axis=1)
    return pmin, np.where(pmax == pmin, (pmin + 1) % 1024, pmax)


def column(T, W, kind):
    """The uniform-width column of (T, W, reference kind): the sweep blocks, then two pair blocks per bit of pair_bits(W)."""
    assert 1 <= W <= T and kind in REFERENCES
    r = reference(T, W, kind)
    rng = np.random.default_rng(seed_of(T, W, kind))
    p = np.arange(1024)
    if W == 1:
        blocks = [sweep_blocks(T, W, r, p, "min", rng), sweep_blocks(T, W, r, p, "max", rng)]
    else:
        blocks = [sweep_blocks(T, W, r, p, "both", rng)]
    n_sweep = sum(b.shape[0] for b in blocks)
    pairs = []
    for j in pair_bits(W):
        for which in ("min", "max"):
            pairs.append((n_sweep + len(pairs), j, which))
            blocks.append(pair_block(T, W, r, j, which, rng)[0][None, :])
    v = np.concatenate(blocks)
    pmin, pmax = designated(v)                                              # a unique extreme is found where it was put
    return Column(T, W, r, v, n_sweep, pmin, pmax, pairs)


def named_masks(n, min_pos, max_pos, seed):
    """name -> bool[n * 1024], None = no mask"""
    rows = np.arange(n)
    at_min, at_max = np.zeros((n, 1024), bool), np.zeros((n, 1024), bool)
    at_min[rows, min_pos] = True
    at_max[rows, max_pos] = True
    return {"all": None,
            "without min": ~at_min.ravel(),
            "without max": ~at_max.ravel(),
            "without both": ~(at_min | at_max).ravel(),
            "only min": at_min.ravel(),
            "only max": at_max.ravel(),
            "min and max only": (at_min | at_max).ravel(),
            "random 50 %": np.random.default_rng(seed).random(n * 1024) < 0.5}


def check_coverage(fields, T, W, r, n_sweep, pairs, wrapping):
    """Conditions 1-4 of the module docstring on np.uint64 fields in index order, asserted on the decoded values (field + r) mod 2^T;
    raises AssertionError naming the first gap."""
    M = U((1 << T) - 1)
    F = np.asarray(fields, dtype=U).reshape(-1, 1024)
    assert W == T or int(F.max()) < (1 << W), "a field wider than W"
    v = (F + U(r)) & M
    p = np.arange(1024)
    s = np.sort(v, axis=1)
    rows = np.arange(1024)
    if W == 1:
        assert n_sweep == 2048
        lo, hi = v[:1024], v[1024:2048]
        assert (lo.argmin(axis=1) == p).all() and (s[:1024, 0] < s[:1024, 1]).all(), ("condition 1", T, W, r, "a minimum is not alone at its position")
        assert (hi.argmax(axis=1) == 1023 - p).all() and (s[1024:2048, -1] > s[1024:2048, -2]).all(), ("condition 1", T, W, r, "a maximum is not alone at its position")
    else:
        assert n_sweep == 1024
        sw, ss = v[:1024], s[:1024]
        assert (sw.argmin(axis=1) == p).all() and (ss[:, 0] < ss[:, 1]).all(), ("condition 1", T, W, r, "a minimum is not alone at its position")
        assert (sw.argmax(axis=1) == 1023 - p).all() and (ss[:, -1] > ss[:, -2]).all(), ("condition 1", T, W, r, "a maximum is not alone at its position")
        lo1, hi1 = ss[:, 0] + U(1), ss[:, -1] - U(1)
        assert (ss[:, 1] == lo1).all(), ("condition 2", T, W, r, "a runner-up is not min + 1")
        assert (ss[:, -2] == hi1).all(), ("condition 2", T, W, r, "a runner-up is not max - 1")
        assert ((sw == lo1[:, None]).sum(axis=1) >= 8).all() and ((sw == hi1[:, None]).sum(axis=1) >= 8).all(), ("condition 2", T, W, r, "fewer than 8 runner-ups")
        near = neighbours(T, 1)
        by_min, by_max = near[p], near[1023 - p]                            # [1024, 4] positions
        min_ok = (sw[rows[:, None], by_min] == lo1[:, None]) | (by_min == (1023 - p)[:, None])
        claimed = (by_max[:, :, None] == by_min[:, None, :]).any(axis=2) | (by_max == p[:, None])
        max_ok = (sw[rows[:, None], by_max] == hi1[:, None]) | claimed
        assert min_ok.all(), ("condition 2", T, W, r, "min + 1 is missing next to a minimum")
        assert max_ok.all(), ("condition 2", T, W, r, "max - 1 is missing next to a maximum")
        crowded = (by_min == (1023 - p)[:, None]).any(axis=1) | claimed.any(axis=1)
        assert crowded.sum() <= MAX_CROWDED, ("condition 2", T, W, r, int(crowded.sum()), "blocks whose extremes crowd each other")
    assert sorted({j for _, j, _ in pairs}) == pair_bits(W) and len(pairs) == 2 * len(pair_bits(W)), ("condition 3", T, W, r, "pair blocks")
    for b, j, which in pairs:
        ext, run = (s[b, 0], s[b, 1]) if which == "min" else (s[b, -1], s[b, -2])
        assert ext != run, ("condition 3", T, W, r, b, "the extreme is not alone")
        assert ((int(ext) - r) ^ (int(run) - r)) & int(M) == 1 << j, ("condition 3", T, W, r, b, f"the fields differ in more than bit {j}")
        at = int(v[b].argmin() if which == "min" else v[b].argmax())
        assert _positions(T)[at, 1] % 2 == 1 and v[b, neighbours(T, 1)[at, 3]] == run, ("condition 3", T, W, r, b, "no runner-up in the even lane before the extreme")
    if wrapping:
        sw, fw = v[:n_sweep], F[:n_sweep]
        wrapped = sw < U(r)
        assert wrapped.any(axis=1).all() and (~wrapped).any(axis=1).all(), ("condition 4", T, W, r, "a block does not cross 2^T")
        assert not wrapped[np.arange(n_sweep), sw.argmax(axis=1)].any(), ("condition 4", T, W, r, "a largest value has wrapped")
        moved = fw[np.arange(n_sweep), sw.argmin(axis=1)] > fw.min(axis=1)
        assert 2 * int(moved.sum()) >= n_sweep, ("condition 4", T, W, r, "the smallest value sits at the smallest field")


def check_column(c, kind):
    check_coverage(c.fields, c.T, c.W, c.r, c.n_sweep, c.pairs, kind == "wrap")


def mixed_tail(T):
    """Widths of the blocks behind the 1024 + T decoded ones: width-0 blocks round a decoded one, inside one group of four."""
    return [0, 1, 0, 0]


def mixed_column(T):
    """The mixed-width column of a type: 1024 + T blocks, block b of width 1 + b mod T carrying the sweep pattern of position b mod 1024
    under the reference kind REFERENCES[b mod 3] of its width (W = 1: min- and max-blocks alternate), then mixed_tail's blocks (the
    width-0 ones hold their reference 1024 times).  Returns (widths uint8[n], references uint64[n], values uint64[n * 1024], min_pos,
    max_pos, the sweep position of each block or -1)."""
    n_dec = 1024 + T
    tail = mixed_tail(T)
    n = n_dec + len(tail)
    rng = np.random.default_rng(98000 + T)
    widths = np.array([1 + b % T for b in range(n_dec)] + tail, dtype=np.uint8)
    decoded = np.flatnonzero(widths > 0)
    kinds = np.arange(n) % 3
    pos = np.where(widths > 0, np.arange(n) % 1024, -1)
    refs = np.zeros(n, dtype=U)
    v = np.empty((n, 1024), dtype=U)
    for b in np.flatnonzero(widths == 0):
        refs[b] = U(int.from_bytes(rng.bytes(8), "little") & ((1 << T) - 1))
        v[b] = refs[b]
    pmin, pmax = np.zeros(n, dtype=np.int64), np.full(n, 1023, dtype=np.int64)
    for W in range(1, T + 1):
        for k, kind in enumerate(REFERENCES):
            sel = decoded[(widths[decoded] == W) & (kinds[decoded] == k)]
            if not sel.size:
                continue
            r = reference(T, W, kind)
            refs[sel] = U(r)
            if W > 1:
                v[sel] = sweep_blocks(T, W, r, pos[sel], "both", rng)
                pmin[sel], pmax[sel] = pos[sel], 1023 - pos[sel]
                continue
            for which in ("min", "max"):
                part = sel[(sel // T) % 2 == (which == "max")]
                if part.size:
                    v[part] = sweep_blocks(T, W, r, pos[part], which, rng)
                    if which == "min":
                        pmin[part], pmax[part] = pos[part], (pos[part] + 1) % 1024
                    else:
                        pmax[part], pmin[part] = 1023 - pos[part], (1024 - pos[part]) % 1024
    return widths, refs, v.reshape(-1), pmin, pmax, pos


def check_mixed_coverage(T, widths, refs, values, pos):
    """Every decoded block of the mixed column: its fields fit its width, its extremes are alone at the positions of its sweep pattern
    and (W >= 2) its runner-ups are min + 1 and max - 1; every width meets at least 1024 // T positions, every position a width."""
    M = U((1 << T) - 1)
    v = values.reshape(-1, 1024)
    s = np.sort(v, axis=1)
    seen = np.zeros(1024, bool)
    for b, W in enumerate(widths):
        W = int(W)
        if W == 0:
            assert (v[b] == refs[b]).all()
            continue
        assert W == T or int(((v[b] - refs[b]) & M).max()) < (1 << W), ("mixed column", T, b, "a field wider than the block's width")
        p = int(pos[b])
        seen[p] = True
        lo_alone, hi_alone = s[b, 0] < s[b, 1] and int(v[b].argmin()) == p, s[b, -1] > s[b, -2] and int(v[b].argmax()) == 1023 - p
        if W == 1:
            assert lo_alone or hi_alone, ("mixed column", T, b)
        else:
            assert lo_alone and hi_alone and s[b, 1] == s[b, 0] + U(1) and s[b, -2] == s[b, -1] - U(1), ("mixed column", T, b)
    assert seen.all()
    for W in range(1, T + 1):
        assert len(set(pos[widths == W])) >= 1024 // T, ("mixed column", T, W)
