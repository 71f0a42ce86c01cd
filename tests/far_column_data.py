"""Far columns: mixed-width columns of two dozen blocks scattered over a packed buffer of 2^33 + 2^20 bytes, so that offsets[b] needs
bit 31, bit 32 and bit 33 -- what tests/test_gpu_far_columns.py hands every `_widths` entry point, and what
tests/test_far_column_data_cpu.py pins without a GPU.  numpy and the oracle only.

The device checks of a mixed-width column ask that offsets[b] is a multiple of 16 and that the block lies inside packed_bytes; offsets
need be neither ascending nor back to back.  The host image of the buffer is therefore sparse: FarBuffer.regions maps a byte offset to
the bytes that lie there (a block of some column, or a decoy); every other byte of the device buffer is noise.

One buffer holds five columns at disjoint offsets (ROLES): the PRIMARY column "a", and the columns a two- or three-column call reads
beside it -- "b", the wide key "key" (the element type's own), the u8 group key "key8" and the set source "src".  The references of
"a" and "b" put pivot(ty) into the middle of every block's range, those of "key" and "src" lie within 60 of each other, so that a
predicate at the pivot and a window over the cluster cannot be answered from a block's reference and width: the block must be read.

The primary column's offset classes (CLASSES), each with at least one block of width > 0:
  plain     offset 0 (width T), and others below 2^31
  bit 31    a block that ends exactly at 2^31 and one that starts there: the sign bit of a 32-bit byte offset
  2^32      variant "edges": a block that ends exactly at 2^32 and one that starts there; variant "straddle": a block whose middle
            lies at 2^32.  Three such blocks cannot be disjoint, hence two variants of the buffer (VARIANTS); everything else is the
            same in both
  alias     a block at o + 2^32, o the offset of ANOTHER plain block of the same width: a kernel that keeps the low half of the offset
            decodes real but wrong data
  bit 33    a block above 2^33
  width 0   one width-0 block at offset 0 and one at exactly packed_bytes (legal: it covers no byte)
and seeded random widths at further offsets of every class, on all eight 16-byte residues mod 128.  The other four columns take
offsets of their own in the same classes (the exact boundaries belong to the primary column: one byte range holds one block).

Decoys: for every block and m = 2^32, 2^31 whose start off mod m differs from off, the block's own bytes COMPLEMENTED are put at
off mod m wherever that range is free.  wrapped_bytes() reads what a kernel would read that computed a block's byte addresses mod m;
the CPU test proves that this is known and decodes to other values for every block of the four far classes."""
import functools

import numpy as np

from datagen import values
from oracle_lib import TYPES, lanes, load_oracle, tbits

B31, B32, B33 = 1 << 31, 1 << 32, 1 << 33
PACKED_BYTES = B33 + (1 << 20)
SLOT = 1 << 14                                   # the spacing of seeded offsets: a block holds at most 8 KiB, a residue at most 112 bytes
N_BLOCKS = 24
VARIANTS = ("edges", "straddle")
ROLES = ("a", "b", "key", "key8", "src")
CLASSES = ("plain", "bit 31", "2^32", "alias", "bit 33", "width 0")
FAR_CLASSES = ("bit 31", "2^32", "alias", "bit 33")
MODULI = (B32, B31)
WINDOW_LO_OFFSET, KEY_SPREAD = 100, 60           # the wide key's references lie 90 .. 150 above 2^(T-1); windows start at 2^(T-1) + 100


def pivot(ty):
    """the value the references of the columns "a" and "b" are laid around: a seeded one of the type's full range"""
    return int(values(ty, 1, 70000 + tbits(ty))[0])


def column_ty(ty, role):
    return "u8" if role == "key8" else ty


def primary_spec(ty, variant):
    """[(class, width, byte offset)] of the primary column's named blocks, in the order of the module's docstring"""
    T = tbits(ty)
    size = lambda w: 128 * w
    spec = [("plain", T, 0), ("width 0", 0, 0), ("plain", T // 2, 1 << 20), ("plain", 1, 3 << 20),
            ("bit 31", T - 1, B31 - size(T - 1)), ("bit 31", T // 2, B31)]
    if variant == "edges":
        spec += [("2^32", T - 1, B32 - size(T - 1)), ("2^32", T // 2 + 1, B32)]
    else:
        spec += [("2^32", T, B32 - size(T) // 2), ("2^32", T // 2 + 1, B32 + (2 << 20) + 48)]
    return spec + [("alias", T // 2, B32 + (1 << 20)), ("bit 33", T, B33 + SLOT + 16), ("width 0", 0, PACKED_BYTES)]


class FarColumn:
    """One column of a FarBuffer: `widths` (uint8), `off` (int64 byte offsets into the buffer), `cls` (the offset class of every
    block), `blocks` [(w, packed elements)] for the oracle, `refs` and `bases`; and its compact copy: the same blocks back to back
    (`compact_off`, `compact`)."""

    def __init__(self, ty, role, cls, widths, off, seed):
        self.ty, self.role, self.n = ty, role, len(widths)
        T, dt = tbits(ty), TYPES[ty][0]
        self.cls = list(cls)
        self.widths = np.asarray(widths).astype(np.uint8)
        self.off = np.asarray(off).astype(np.int64)
        self.sizes = self.widths.astype(np.int64) * 128
        esz = T // 8
        self.blocks = [(int(w), values(ty, 128 * int(w) // esz, seed + 1 + b)) for b, w in enumerate(self.widths)]
        N = 1 << T
        if role in ("key", "src"):               # clustered: a window of a few dozen slots holds the narrow blocks' values
            rs = np.random.default_rng(seed)
            self.refs = np.array([(N // 2 + 90 + int(x)) % N for x in rs.integers(0, KEY_SPREAD, size=self.n)], dtype=np.uint64).astype(dt)
        elif role in ("a", "b"):                 # every block's range [r, r + 2^w) has pivot(ty) in its middle: no constant near the pivot
            K = pivot(ty)                        # decides a block of width > 0 from its reference and width alone
            self.refs = np.array([(K - ((1 << int(w)) >> 1)) % N for w in self.widths], dtype=np.uint64).astype(dt)
        else:
            self.refs = values(ty, self.n, seed + 100)
        self.bases = values(ty, self.n * lanes(ty), seed + 101)
        self.compact_off = (np.cumsum(self.sizes) - self.sizes).astype(np.int64)
        self.compact = np.concatenate([pk for _, pk in self.blocks]) if self.n else np.zeros(0, dt)

    def block_bytes(self, b):
        return self.blocks[b][1].view(np.uint8)

    @functools.cached_property
    def unpack(self):
        o = load_oracle()
        return np.concatenate([o.unpack(self.ty, w, pk) for w, pk in self.blocks])

    @functools.cached_property
    def unfor(self):
        o = load_oracle()
        return np.concatenate([o.unfor_pack(self.ty, w, pk, self.refs[b]) for b, (w, pk) in enumerate(self.blocks)])

    @functools.cached_property
    def undelta(self):
        """in transposed order, as the reference leaves it"""
        o, L = load_oracle(), lanes(self.ty)
        return np.concatenate([o.undelta_pack(self.ty, w, pk, self.bases[b * L:(b + 1) * L]) for b, (w, pk) in enumerate(self.blocks)])

    @functools.cached_property
    def undelta_rows(self):
        """in original row order"""
        return load_oracle().batch("untranspose", self.ty, None, self.undelta)


def _primary(ty, variant, slots):
    T = tbits(ty)
    spec = primary_spec(ty, variant)
    rs = np.random.default_rng(71000 + T)
    cycle = ("bit 31", "2^32", "bit 33", "plain", "2^32")
    base = {"plain": 0, "bit 31": B31, "2^32": B32}
    for i in range(len(spec), N_BLOCKS):
        c, w, res = cycle[i % len(cycle)], int(rs.integers(0, T + 1)), 16 * (i % 8)
        off = B33 + next(slots) * SLOT + res if c == "bit 33" else base[c] + (1 << 24) + i * SLOT + res
        spec.append((c if w else "width 0", w, off))
    order = np.random.default_rng(71100 + T).permutation(len(spec))
    spec = [spec[i] for i in order]
    return FarColumn(ty, "a", [s[0] for s in spec], [s[1] for s in spec], [s[2] for s in spec], 72000 + 1000 * T)


def _secondary(ty, role, slots):
    """plain, bit 31, 2^32, alias (of the plain block three in front of it), bit 33, 2^32, and so on; the widths 0, 1, T/2, T - 1 and T
    at far offsets, seeded random ones elsewhere"""
    cty, r = column_ty(ty, role), ROLES.index(role)
    T = tbits(cty)
    rs = np.random.default_rng(73000 + 10 * T + r)
    cycle = ("plain", "bit 31", "2^32", "alias", "bit 33", "2^32")
    widths = [int(w) for w in rs.integers(0, T + 1, size=N_BLOCKS)]
    for i, w in zip((1, 2, 4, 5, 8), (0, 1, T // 2, T - 1, T)):
        widths[i] = w
    cls, off = [], []
    for i in range(N_BLOCKS):
        c, res = cycle[i % len(cycle)], 16 * ((i + r) % 8)
        low = ((r + 1) << 24) + i * SLOT + res
        if c == "plain":
            widths[i] = max(widths[i], 1)
            o = low
        elif c == "alias":
            widths[i] = widths[i - 3]
            o = off[i - 3] + B32
        elif c == "bit 33":
            o = B33 + next(slots) * SLOT + res
        else:
            o = {"bit 31": B31, "2^32": B32}[c] + low
        cls.append(c if widths[i] else "width 0")
        off.append(o)
    return FarColumn(cty, role, cls, widths, off, 74000 + 1000 * T + 100 * r)


class FarBuffer:
    """The sparse host image of one packed buffer of PACKED_BYTES bytes of element type `ty`: `columns` role -> FarColumn, `regions`
    byte offset -> uint8 bytes (every block of width > 0 of every column, and every decoy), `decoys` the decoys' offsets."""

    def __init__(self, ty, variant):
        assert variant in VARIANTS
        self.ty, self.variant = ty, variant
        slots = iter(range(2, 64))               # 16-KiB slots above 2^33 (slot 1: the primary column's named block)
        self.columns = {"a": _primary(ty, variant, slots)}
        for role in ROLES[1:]:
            self.columns[role] = _secondary(ty, role, slots)
        self.regions, self.owner = {}, {}
        for role, c in self.columns.items():
            for b in range(c.n):
                if c.widths[b]:
                    assert self.free(int(c.off[b]), int(c.sizes[b])), (ty, variant, role, b, "two blocks overlap")
                    self.regions[int(c.off[b])] = c.block_bytes(b)
                    self.owner[int(c.off[b])] = (role, b)
        self.decoys = []
        for role, c in self.columns.items():
            for b in range(c.n):
                off, size = int(c.off[b]), int(c.sizes[b])
                for m in MODULI:
                    s = off % m
                    if size and s != off and s + size <= PACKED_BYTES and self.free(s, size):
                        self.regions[s] = ~c.block_bytes(b)
                        self.owner[s] = ("decoy of", role, b)
                        self.decoys.append(s)
        self._starts = np.array(sorted(self.regions), dtype=np.int64)

    def free(self, start, size):
        return all(start + size <= o or o + len(r) <= start for o, r in self.regions.items())

    def read(self, start, size):
        """the bytes [start, start + size) where ONE region holds all of them, else None (the device holds noise there)"""
        i = int(np.searchsorted(self._starts, start, side="right")) - 1
        if i < 0:
            return None
        o = int(self._starts[i])
        r = self.regions[o]
        return r[start - o:start - o + size] if start + size <= o + len(r) else None

    def wrapped_bytes(self, off, size, m):
        """what lies at the addresses (off + i) mod m, i < size: the block as a kernel sees it that keeps its byte addresses mod m;
        None where any of it is unknown"""
        parts, a = [], off
        while a < off + size:
            step = min(off + size - a, m - a % m)
            part = self.read(a % m, step)
            if part is None:
                return None
            parts.append(part)
            a += step
        return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def far_buffer(ty, variant):
    return FarBuffer(ty, variant)
