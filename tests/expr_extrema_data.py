"""Column PAIRS in which ONE row decides the minimum or the maximum of x = a o b (o: '*', '+', '-'), and single blocks that hold the
largest sums a block can, for the kernels that aggregate an expression between two packed columns (unfor_aggregate_columns,
unfor_aggregate_columns_widths, unfor_aggregate_by_columns).  x is group_columns_data.expr: both values zero-extended, the operation
mod 2^64.  Everything is built from the VALUES; numpy only, nothing here packs or unpacks.

SWEEP o CONSTANT ('*' and '+').  One side is extrema_data.column(T, W, kind) -- 1024 sweep blocks (2048 at W = 1) and the pair blocks
-- the other holds one value c in every row; either column may be the sweeping one (the GPU tests run both roles), and the constant
side is packed in two ways (constant_side): width 0 with the reference c, or a width >= 1 with equal fields and a nonzero reference.
check_sweep asserts on x, for every (T, W, kind, op, c) that sweep_plan hands out:
 1. every sweep block holds a unique minimum and a unique maximum of x (W = 1: the min-blocks a unique minimum, the max-blocks a
    unique maximum);
 2. over the sweep blocks every one of the 1024 index-order positions is the unique minimum of some block and the unique maximum of
    some block;
 3. where `stepped` claims it (W >= 2) the runner-up differs from the extreme by the op's
    smallest step: c for '*', 1 for '+'.
For T <= 32 no x wraps, x grows with the sweeping value and the conditions follow from extrema_data's own; the u64 combinations whose
sums or products wrap past 2^64 and move the extremes are left out by `admissible` (tests/test_expr_extrema_data_cpu.py holds the
list).  c = 2^(T-1) under '*' (T <= 32, the `zero` columns) makes x = a << (T - 1): the pair blocks then set their two leading values
apart in bit j + T - 1 of x alone (HIGH_BITS: the bits round the 16- and 32-bit edges of the narrow accumulators).

'-' ACROSS ZERO (zero_crossing).  Blocks built from signed target differences d: b seeded, a = b + d, both inside the type; every
block is packed at the width its own span needs with its minimum as the reference.  Block p of a column of 1024:
 * d = 0 exactly once, at position p: the unsigned minimum of the patterns;
 * d = +1 at least 8 times, in the four extrema_data.neighbours(T, 1) of p among them;
 * d = -1 exactly once, at position 1023 - p: the unsigned maximum, 2^64 - 1;
 * d = -2 at least 8 times, in the neighbours of 1023 - p among them (but where such a cell is p or one of its neighbours, which go
   first: extrema_data.MAX_CROWDED blocks at the most);
 * every other row has 3 <= |d| <= span, and both signs occur.
Three spans per type -- 3, 2^(T/2), 2^T - 1 -- give narrow, middle and full-width blocks.  Three more blocks behind the widest column
hold d = -(2^T - 1) (a = 0, b = 2^T - 1) among small positive d, d = +(2^T - 1) among small negative d, and both among small d of
both signs.

LARGEST SUMS (largest_sums).  T in {8, 16}: single blocks whose 1024 rows all hold the extreme operands (a = b = 2^T - 1 for '*' and
'+'; a = 0, b = 2^T - 1 and the reverse for '-'), each through the four routes (both sides packed at W = T, either side width 0,
both width 0).  The expected slot comes from python integers mod 2^64."""
import numpy as np

import extrema_data as ed
from group_columns_data import expr

U = np.uint64
OPS = ["*", "+", "-"]
SPANS = ("narrow", "middle", "full")
PACKINGS = ("width 0", "packed")
HIGH_BITS = {8: (7, 8, 14), 16: (15, 16, 30), 32: (31, 32, 33, 62)}         # bits of x the c = 2^(T-1) pair blocks must reach


# ---------------------------------------------------------------------------------------------------------------------------------
# sweep o constant
# ---------------------------------------------------------------------------------------------------------------------------------
def constants(T, op):
    """the candidates c of (T, op): 1, 3 and (T <= 32) the type's largest value"""
    assert op in ("*", "+")
    return (1, 3, (1 << T) - 1) if T <= 32 else (1, 3)


def sweep_widths(T):
    """the widths of the sweeping side, per (type, op)"""
    return (2, T // 2 + 1, T)


def admissible(T, W, kind, op, c):
    """Do conditions 1 - 3 hold for the combination?  Always below 64 bits; at 64 bits not where x wraps past 2^64 inside a block."""
    if T < 64 or (op == "*" and c == 1):
        return True
    if op == "*":
        return not (W == 63 and kind in ("zero", "mid"))
    return kind in ("zero", "mid") and W < 64


def candidates(T, op):
    """Every (W, kind, c) the plan of (T, op) is drawn from.  The three widths, each under one reference kind and one constant, so that
    every kind and every constant occurs per (type, op): '*' takes (2, wrap), (T/2 + 1, mid), (T, zero), '+' takes (2, mid),
    (T/2 + 1, zero), (T, wrap).  '*' below 64 bits adds c = 2^(T-1) on the `zero` column of every width, W = 1 comes once per type
    (under '*'), and u32 adds W = 3 for bit 33 of HIGH_BITS."""
    cs = constants(T, op)
    kinds = ("wrap", "mid", "zero") if op == "*" else ("mid", "zero", "wrap")
    out = []
    for wi, W in enumerate(sweep_widths(T)):
        out.append((W, kinds[wi], cs[(wi + (op == "*")) % len(cs)]))
        if op == "*" and T <= 32:
            out.append((W, "zero", 1 << (T - 1)))
    if op == "*":
        out.append((1, "mid", 3))
        if T == 32:
            out.append((3, "zero", 1 << 31))
    return out


def sweep_plan(T, op):
    """[(W, kind, c, packing of the constant side when column a sweeps, packing when column b sweeps)]: the admissible candidates; both
    roles run on every one of them, with the two packings swapped from one combination to the next."""
    plan = [k for k in candidates(T, op) if admissible(T, *k[:2], op, k[2])]
    return [(W, kind, c, PACKINGS[i % 2], PACKINGS[1 - i % 2]) for i, (W, kind, c) in enumerate(plan)]


def left_out(T, op):
    return [k for k in candidates(T, op) if not admissible(T, *k[:2], op, k[2])]


def constant_side(T, c, packing):
    """(width, reference, field): a column that decodes to c in every row -- width 0 with the reference c, or width 3 / T (c odd / even)
    with the field 5 in every row under the reference c - 5 mod 2^T, which is never 0 for the constants used here and wraps for c < 5."""
    if packing == "width 0":
        return 0, c, 0
    r = (c - 5) % (1 << T)
    assert r != 0
    return (3 if c % 2 else T), r, 5


def stepped(W):
    """condition 3 is claimed from W = 2 up, as extrema_data claims its own runner-ups"""
    return W >= 2


def check_sweep(T, W, op, c, col, x):
    """Conditions 1 - 3 of the module docstring on x = expr(op, sweep, c) (uint64, index order, the whole column of extrema_data.column);
    raises AssertionError naming the first gap.  Returns (min_pos, max_pos) of every block, taken from x."""
    what = (T, W, op, c, col.r)
    xb = x.reshape(col.n, 1024)
    s = np.sort(xb, axis=1)
    pmin, pmax = ed.designated(xb)
    lo_alone, hi_alone = s[:, 0] < s[:, 1], s[:, -1] > s[:, -2]
    if W == 1:
        assert col.n_sweep == 2048
        assert lo_alone[:1024].all() and hi_alone[1024:2048].all(), ("condition 1", what)
        assert sorted(pmin[:1024]) == list(range(1024)) and sorted(pmax[1024:2048]) == list(range(1024)), ("condition 2", what)
    else:
        n = col.n_sweep
        assert n == 1024 and lo_alone[:n].all() and hi_alone[:n].all(), ("condition 1", what)
        assert sorted(pmin[:n]) == list(range(1024)) and sorted(pmax[:n]) == list(range(1024)), ("condition 2", what)
        if stepped(W):
            step = U(c if op == "*" else 1)
            assert (s[:n, 1] - s[:n, 0] == step).all() and (s[:n, -1] - s[:n, -2] == step).all(), ("condition 3", what)
    return pmin, pmax


def high_bits_reached(T):
    """the bits of x in which the extreme and its runner-up of a pair block differ ALONE, over the c = 2^(T-1) combinations of the plan"""
    seen = set()
    for W, kind, c, _, _ in sweep_plan(T, "*"):
        if c == 1 << (T - 1) and W > 1:
            col = ed.column(T, W, kind)
            xb = np.sort(expr("*", col.values, U(c)).reshape(col.n, 1024), axis=1)
            for b, _, which in col.pairs:
                diff = int(xb[b, 0] ^ xb[b, 1]) if which == "min" else int(xb[b, -1] ^ xb[b, -2])
                if diff & (diff - 1) == 0:
                    seen.add(diff.bit_length() - 1)
    return seen


# ---------------------------------------------------------------------------------------------------------------------------------
# the mixed-width pair of a type
# ---------------------------------------------------------------------------------------------------------------------------------
MIXED_TAIL = [0, 2, 0, 0]                                                   # width-0 blocks round a decoded one, inside one group of four


def mixed_widths(T, op):
    """the cycle of the sweeping side's widths; 5 of them, so 1024 blocks meet every (width, position mod 5) once in five rounds"""
    return (2, T // 2 + 1, T - 1, 3, T) if not (T == 64 and op == "+") else (2, 33, 63, 3, 17)


def mixed_kinds(T, op):
    return ed.REFERENCES if not (T == 64 and op == "+") else ("zero", "mid")


class MixedPair:
    """widths / refs / values of the sweeping column and cw / cr / cvalues of the constant one, per block (values uint64[n * 1024] in
    index order); c: the constant of each block; pos: the sweep position of each decoded block or -1; x and (min_pos, max_pos) taken
    from it."""


def mixed_pair(T, op):
    """The mixed-width pair of (T, op), '*' or '+': 1024 blocks, block b carrying the sweep pattern of position b (its minimum there, its
    maximum at 1023 - b) at the width mixed_widths[b mod 5] under the reference kind of (b div 5) mod 3, then MIXED_TAIL's blocks (a
    width-0 block of the sweeping side holds its reference 1024 times).  The constant side of block b holds constants(T, op)[b mod 3]
    (u64: mod 2) -- 1 under u64 '+' / '*' where 3 is not admissible -- packed as width 0 in the even blocks and with equal fields in the
    odd ones: width-0 blocks stand next to decoded ones on both sides, and the tail meets (0, 0), (0, w), (w, 0) and (w, w')."""
    m = MixedPair()
    wl, kl, cs = mixed_widths(T, op), mixed_kinds(T, op), constants(T, op)
    n = 1024 + len(MIXED_TAIL)
    rng = np.random.default_rng(97000 + T + 7 * OPS.index(op))
    m.T, m.op, m.n = T, op, n
    m.widths = np.array([wl[b % 5] for b in range(1024)] + MIXED_TAIL, dtype=np.uint8)
    kinds = [kl[(b // 5) % len(kl)] for b in range(1024)] + ["zero", "mid", "zero", "zero"]
    m.pos = np.where(m.widths > 0, np.arange(n) % 1024, -1)
    m.refs = np.zeros(n, dtype=U)
    v = np.empty((n, 1024), dtype=U)
    for b in np.flatnonzero(m.widths == 0):
        m.refs[b] = U(int.from_bytes(rng.bytes(8), "little") & ((1 << T) - 1) & ~(3 << (T - 2)))    # (below 2^(T-2): + 3 cannot wrap)
        v[b] = m.refs[b]
    for W in sorted(set(int(w) for w in m.widths if w)):
        for kind in kl:
            sel = np.array([b for b in range(n) if m.widths[b] == W and kinds[b] == kind], dtype=np.int64)
            if sel.size:
                r = ed.reference(T, W, kind)
                m.refs[sel] = U(r)
                v[sel] = ed.sweep_blocks(T, W, r, m.pos[sel], "both", rng)
    m.values = v.reshape(-1)
    c = np.array([cs[b % len(cs)] for b in range(n)], dtype=U)
    for b in range(n):
        if m.widths[b] and not admissible(T, int(m.widths[b]), kinds[b], op, int(c[b])):
            c[b] = U(1)
            assert admissible(T, int(m.widths[b]), kinds[b], op, 1), (T, op, b)
    m.c = c
    sides = [constant_side(T, int(c[b]), PACKINGS[b % 2]) for b in range(n)]
    m.cw = np.array([s[0] for s in sides], dtype=np.uint8)
    m.cr = np.array([s[1] for s in sides], dtype=U)
    m.cvalues = np.repeat(c, 1024)
    m.x = expr(op, m.values, m.cvalues)
    m.min_pos, m.max_pos = ed.designated(m.x.reshape(n, 1024))
    return m


def check_mixed_pair(m):
    """every decoded block of the sweeping side: x has its unique minimum at the block's sweep position and its unique maximum opposite,
    the runner-ups one step away; every position and every width occurs"""
    xb = m.x.reshape(m.n, 1024)
    s = np.sort(xb, axis=1)
    dec = np.flatnonzero(m.widths > 0)
    assert (s[dec, 0] < s[dec, 1]).all() and (s[dec, -1] > s[dec, -2]).all(), ("mixed pair", m.T, m.op, "an extreme is not alone")
    assert (m.min_pos[dec] == m.pos[dec]).all() and (m.max_pos[dec] == 1023 - m.pos[dec]).all(), ("mixed pair", m.T, m.op, "an extreme moved")
    step = m.c[dec] if m.op == "*" else U(1)
    assert (s[dec, 1] - s[dec, 0] == step).all() and (s[dec, -1] - s[dec, -2] == step).all(), ("mixed pair", m.T, m.op, "a runner-up is further off")
    assert set(m.pos[dec]) == set(range(1024)) and set(m.widths[:1024]) == set(mixed_widths(m.T, m.op))
    both = {(min(int(a), 1), min(int(b), 1)) for a, b in zip(m.widths, m.cw)}
    assert both == {(0, 0), (0, 1), (1, 0), (1, 1)}, ("mixed pair", m.T, m.op, "a route is missing", both)


# ---------------------------------------------------------------------------------------------------------------------------------
# '-' across zero
# ---------------------------------------------------------------------------------------------------------------------------------
def span_of(T, which):
    return {"narrow": 3, "middle": 1 << (T // 2), "full": (1 << T) - 1}[which]


class Crossing:
    """a / b: uint64[n * 1024] values in index order; d_min / d_max: the position of d = 0 and of d = -1 in each of the first n_sweep
    blocks; x = a - b mod 2^64 and (min_pos, max_pos) taken from it; wa / wb / ra / rb: the width each block's own span needs and its
    minimum, per block."""


def _differences(T, S, positions, rng):
    """[n, 1024] (b, a = b + d): see the module docstring"""
    n = positions.size
    M = (1 << T) - 1
    rows = np.arange(n)
    raw = lambda: np.frombuffer(rng.bytes(8 * n * 1024), dtype=U).reshape(n, 1024)
    if S < M:                                                               # b in a window of S + 1 values with room for +-S round it
        base = U(S) + np.frombuffer(rng.bytes(8 * n), dtype=U) % U(M - 3 * S)
        b = base[:, None] + raw() % U(S + 1)
    else:                                                                   # anywhere that leaves room for |d| = 3 on both sides
        b = U(3) + raw() % U(M - 5)
    up = np.minimum(U(S), U(M) - b)                                         # the largest d and the largest -d of the row
    down = np.minimum(U(S), b)
    neg = rng.integers(0, 2, size=(n, 1024)).astype(bool)
    mag = U(3) + raw() % (np.where(neg, down, up) - U(2))
    a = np.where(neg, b - mag, b + mag)
    pmin, pmax = positions, 1023 - positions
    near, far = ed.neighbours(T, 1), ed.neighbours(T, 2)
    anywhere = rng.integers(0, 1024, size=(2, n, 12))                       # a dozen runner-ups more, wherever
    for nb, neg_, m_ in ((anywhere[0], True, 2), (anywhere[1], False, 1),
                         (far[pmax], True, 2), (far[pmin], False, 1), (near[pmax], True, 2), (near[pmin], False, 1)):    # the later ones go first
        a[rows[:, None], nb] = b[rows[:, None], nb] - U(m_) if neg_ else b[rows[:, None], nb] + U(m_)
    a[rows, pmax] = b[rows, pmax] - U(1)
    a[rows, pmin] = b[rows, pmin]
    return a, b


def _edge_blocks(T, rng):
    """three blocks round d = -(2^T - 1) and d = +(2^T - 1): the first among d in 2..8, the second among d in -8..-2, both among both"""
    M = (1 << T) - 1
    out_a, out_b = [], []
    for i, signs in enumerate(((1,), (-1,), (1, -1))):
        b = 16 + np.frombuffer(rng.bytes(8 * 1024), dtype=U) % U(M - 32)
        mag = U(2) + np.frombuffer(rng.bytes(8 * 1024), dtype=U) % U(7)
        neg = rng.integers(0, 2, size=1024).astype(bool) if len(signs) == 2 else np.full(1024, signs[0] < 0)
        a = np.where(neg, b - mag, b + mag)
        at = rng.choice(1024, size=2, replace=False)
        if i != 1:
            a[at[0]], b[at[0]] = U(0), U(M)                                 # d = -(2^T - 1)
        if i != 0:
            a[at[1]], b[at[1]] = U(M), U(0)                                 # d = +(2^T - 1)
        out_a.append(a)
        out_b.append(b)
    return np.stack(out_a), np.stack(out_b)


def _block_packing(T, v):
    """(width, reference) per block of [n, 1024] values: the bits of the block's span, its minimum"""
    lo, hi = v.min(axis=1), v.max(axis=1)
    return np.array([int(int(h) - int(l)).bit_length() for l, h in zip(lo, hi)], dtype=np.uint8), lo


def zero_crossing(T, which):
    """The '-' column pair of (T, span): 1024 blocks, block p with d = 0 at p and d = -1 at 1023 - p; behind the `full` one the three
    blocks of _edge_blocks."""
    S = span_of(T, which)
    rng = np.random.default_rng(96000 + 10 * T + SPANS.index(which))
    a, b = _differences(T, S, np.arange(1024), rng)
    if which == "full":
        ea, eb = _edge_blocks(T, rng)
        a, b = np.concatenate([a, ea]), np.concatenate([b, eb])
    z = Crossing()
    z.T, z.S, z.n, z.n_sweep = T, S, a.shape[0], 1024
    z.wa, z.ra = _block_packing(T, a)
    z.wb, z.rb = _block_packing(T, b)
    z.a, z.b = a.reshape(-1), b.reshape(-1)
    z.x = expr("-", z.a, z.b)
    z.min_pos, z.max_pos = ed.designated(z.x.reshape(z.n, 1024))
    return z


def signed(x):
    """the uint64 patterns as python-exact signed differences (int64 holds every d of T <= 32; for u64 the pattern IS the definition)"""
    return x.view(np.int64)


def check_crossing(z):
    """the conditions of the module docstring on z.x; raises AssertionError naming the first gap"""
    T, what = z.T, (z.T, z.S)
    M = (1 << T) - 1
    assert int(z.a.max()) <= M and int(z.b.max()) <= M, ("a value outside the type", what)
    xb = z.x.reshape(z.n, 1024)[:1024]
    p = np.arange(1024)
    rows = p
    assert ((xb == U(0)).sum(axis=1) == 1).all() and (xb[rows, p] == U(0)).all(), ("d = 0 is not alone at its position", what)
    assert ((xb == U(2 ** 64 - 1)).sum(axis=1) == 1).all() and (xb[rows, 1023 - p] == U(2 ** 64 - 1)).all(), ("d = -1 is not alone at its position", what)
    assert (z.min_pos[:1024] == p).all() and (z.max_pos[:1024] == 1023 - p).all()
    assert ((xb == U(1)).sum(axis=1) >= 8).all() and ((xb == U(2 ** 64 - 2)).sum(axis=1) >= 8).all(), ("fewer than 8 runner-ups", what)
    near = ed.neighbours(T, 1)
    by_min, by_max = near[p], near[1023 - p]
    min_ok = (xb[rows[:, None], by_min] == U(1)) | (by_min == (1023 - p)[:, None])
    claimed = (by_max[:, :, None] == by_min[:, None, :]).any(axis=2) | (by_max == p[:, None])
    max_ok = (xb[rows[:, None], by_max] == U(2 ** 64 - 2)) | claimed
    assert min_ok.all(), ("d = +1 is missing next to d = 0", what)
    assert max_ok.all(), ("d = -2 is missing next to d = -1", what)
    crowded = (by_min == (1023 - p)[:, None]).any(axis=1) | claimed.any(axis=1)
    assert crowded.sum() <= ed.MAX_CROWDED, (int(crowded.sum()), "blocks whose extremes crowd each other", what)
    if T < 64:                                                              # |d| as a number: the sign-extended pattern
        d = signed(xb)
        rest = (np.abs(d) >= 3)
        assert (rest | np.isin(d, (0, 1, -1, -2))).all() and int(np.abs(d).max()) <= z.S, ("a difference outside 3 .. span", what)
        assert ((d >= 3).sum(axis=1) > 0).all() and ((d <= -3).sum(axis=1) > 0).all(), ("one sign is missing", what)
    else:                                                                   # u64: a < b and a > b both occur beyond the placed rows
        a, b = z.a.reshape(z.n, 1024)[:1024], z.b.reshape(z.n, 1024)[:1024]
        far_up, far_down = (a > b) & (a - b >= U(3)), (a < b) & (b - a >= U(3))
        assert (far_up.sum(axis=1) > 0).all() and (far_down.sum(axis=1) > 0).all(), ("one sign is missing", what)
        assert (far_up | far_down | np.isin(xb, (U(0), U(1), U(2 ** 64 - 1), U(2 ** 64 - 2)))).all()
    # the blocks are packed at their own span: the widths a span is meant to give occur
    fits = lambda v, w, r: all(int((v.reshape(z.n, 1024)[i] - r[i]).max()) < (1 << int(w[i])) or int(w[i]) == 64 for i in range(z.n))
    assert fits(z.a, z.wa, z.ra) and fits(z.b, z.wb, z.rb)
    if z.S == 3:
        assert int(z.wb.max()) <= 2 and int(z.wa.max()) <= 4, ("the narrow span is not narrow", what, int(z.wa.max()), int(z.wb.max()))
    elif z.S == M:
        assert int(z.wa.min()) >= T - 1 and int(z.wb.min()) >= T - 1, ("the full span is not full", what)
        e = z.n - 3
        ea, eb = z.a.reshape(z.n, 1024)[e:], z.b.reshape(z.n, 1024)[e:]
        down, up = (ea == U(0)) & (eb == U(M)), (ea == U(M)) & (eb == U(0))
        assert [int(k.sum()) for k in down] == [1, 0, 1] and [int(k.sum()) for k in up] == [0, 1, 1], ("the edge blocks", what)
    else:
        assert T // 2 <= int(z.wb.min()) and int(z.wa.max()) <= T // 2 + 2 < T, ("the middle span is not in the middle", what)


# ---------------------------------------------------------------------------------------------------------------------------------
# the largest sums a block can hold
# ---------------------------------------------------------------------------------------------------------------------------------
ROUTES = ((1, 1), (0, 1), (1, 0), (0, 0))                                   # is side a / side b packed (at W = T), or width 0


def largest_sums(T):
    """[(op, a, b, [count, sum, min, max] mod 2^64 from python integers)]: the extreme operands in all 1024 rows"""
    M = (1 << T) - 1
    out = []
    for op, a, b in (("*", M, M), ("+", M, M), ("-", 0, M), ("-", M, 0)):
        x = (a * b if op == "*" else a + b if op == "+" else a - b)
        out.append((op, a, b, [1024, (1024 * x) % 2 ** 64, x % 2 ** 64, x % 2 ** 64]))
    return out


def side(T, value, packed):
    """(width, reference) of a block that holds `value` 1024 times: W = T under the reference 0, or width 0 under the reference"""
    return (T, 0) if packed else (0, value)
