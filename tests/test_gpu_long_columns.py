"""GPU: every column consumer over a LONG column -- u8 at W = 1 in the uniform forms, 4 300 000 blocks = 4.403e9 rows, under a mask that
keeps 4.369e9 of them -- so that the row index, the running output offset of the select kernels (inside the column, not only at its
end), fl_mask_offsets' prefix sum and total, the 64-bit count of an aggregate, of one group and of one window slot, and the hit / miss
and inside / outside counters all pass 2^32.  A 32-bit `blk * 1024`, an `unsigned` count or a 32-bit out_offsets[b] fails here.

The column: packed bytes from fl_fill_random, refs[b] = b % 200, Delta bases from a seeded torch generator; the mask is all ones except
in the blocks with b % 64 == 0, which carry random words.  The reference is computed on the device by torch in exact int64 over the
column as FoR.unfor_pack / Delta.undelta_pack_untranspose decode it, in chunks of 2^28 rows; the decoded column itself, and the
sampled blocks of every per-block output, are pinned against the oracle on about 200 blocks: the first and the last, 2^22 - 1 and
2^22 (row 2^32), the block in which out_offsets crosses 2^32, masked blocks and random others."""
import ctypes

import numpy as np
import pytest

import columns_data
import delta_compare_range_data as dd
import gpu_support as gs
import test_gpu_for_compare_in as cin
import test_gpu_for_compare_range as rng_
from gpu_support import fl  # noqa: F401 (fixture)
from gpu_support import GUARD, SENTINEL, to_dev
from oracle_lib import load_oracle

pytestmark = pytest.mark.gpu

N = 4_300_000
ROWS = N * 1024
CHUNK = 1 << 18                                 # blocks per chunk of the reference: 2^28 rows
BIG = 1 << 62
I64_MINUS_1 = -1                                # the bits of 2^64 - 1: the identity of min
LO, HI = 50, 120                                # the interval of the range predicates
MEMBERS = [3, 77, 78, 150, 199]
SLOTS = 199                                     # the lookup table and the set window: keys 199 and 200 (0.75 % of the rows) miss


class Column:
    def __init__(self, fl):
        import torch
        self.fl, self.torch = fl, torch
        dev = "cuda:0"
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.pk, self.pk_b = (torch.empty(N * 128, dtype=torch.uint8, device=dev) for _ in range(2))
        for t, seed in ((self.pk, 91), (self.pk_b, 92)):
            assert fl.load().fl_fill_random(t.data_ptr(), t.numel(), seed, stream) == 0
        b = np.arange(N)
        self.refs_np = (b % 200).astype(np.uint8)
        self.refs_b_np = ((b % 200) + (b // 200) % 3 - 1).astype(np.uint8)         # a's reference - 1, + 0, + 1 (mod 256): a < b is open
        self.key_refs_np = (b % 5).astype(np.uint8)                                # a W = 1 key column over pk_b: keys 0 .. 5
        self.refs, self.refs_b, self.key_refs = to_dev(self.refs_np), to_dev(self.refs_b_np), to_dev(self.key_refs_np)
        g = torch.Generator(device=dev).manual_seed(9100)
        self.bases = torch.randint(0, 256, (N * 128,), dtype=torch.uint8, device=dev, generator=g)
        words = torch.full((N, 32), -1, dtype=torch.int32, device=dev)
        words[::64] = torch.randint(-(1 << 31), 1 << 31, ((N + 63) // 64, 32), dtype=torch.int32, device=dev, generator=g)
        self.words = words.view(-1)
        self.pop = self.popcounts(self.words)
        self.kept = int(self.pop.sum().item())
        self.pop_np = self.pop.cpu().numpy()
        self.oo_np = np.cumsum(self.pop_np) - self.pop_np
        self.cross = int(np.searchsorted(self.oo_np, 1 << 32, side="right")) - 1  # the block whose run holds output element 2^32
        rng = np.random.default_rng(9101)
        picks = np.concatenate([[0, 1, 63, 64, 65, N - 1, N - 2, (1 << 22) - 1, 1 << 22, self.cross - 1, self.cross, self.cross + 1],
                                rng.integers(0, N, size=160), rng.integers(0, N // 64, size=30) * 64])
        self.picks = np.unique(picks[(picks >= 0) & (picks < N)])
        self.d_picks = to_dev(self.picks.astype(np.int64))
        self.pk_s, self.pk_b_s = (t.view(N, 128)[self.d_picks].cpu().numpy() for t in (self.pk, self.pk_b))
        self.bases_s = self.bases.view(N, 128)[self.d_picks].cpu().numpy()
        self.words_s = self.sample(self.words, 32).view(np.int32)
        self.keep_s = np.unpackbits(self.words_s.view(np.uint8), bitorder="little").astype(bool).reshape(-1, 1024)
        o = load_oracle()
        self.a_s = np.stack([o.unfor_pack("u8", 1, self.pk_s[j], int(self.refs_np[b])) for j, b in enumerate(self.picks)])
        self.b_s = np.stack([o.unfor_pack("u8", 1, self.pk_b_s[j], int(self.refs_b_np[b])) for j, b in enumerate(self.picks)])
        self.key_s = np.stack([o.unfor_pack("u8", 1, self.pk_b_s[j], int(self.key_refs_np[b])) for j, b in enumerate(self.picks)])
        self.d_s = np.stack([o.untranspose("u8", o.undelta_pack("u8", 1, self.pk_s[j], self.bases_s[j])) for j in range(len(self.picks))])
        self._decoded = {}

    # ---- the column as the library's own decoders give it, pinned against the oracle on the sample ----
    def decoded(self, which):
        """"a" / "b" / "key": FoR.unfor_pack of the column; "delta": Delta.undelta_pack_untranspose -- u8[ROWS], kept"""
        if which not in self._decoded:
            fl = self.fl
            if which == "delta":
                v, want = fl.Delta.undelta_pack_untranspose(1, self.pk, self.bases), self.d_s
            else:
                pk, refs, want = {"a": (self.pk, self.refs, self.a_s), "b": (self.pk_b, self.refs_b, self.b_s), "key": (self.pk_b, self.key_refs, self.key_s)}[which]
                v = fl.FoR.unfor_pack(1, pk, refs)
            assert v.numel() == ROWS
            assert np.array_equal(self.sample(v, 1024), want), (which, "the decoded column differs from the oracle's on the sampled blocks")
            self._decoded[which] = v
        return self._decoded[which]

    def drop(self, *which):
        for w in which:
            self._decoded.pop(w, None)

    def sample(self, t, per_block):
        """the sampled blocks of a per-block device tensor, as numpy [len(picks), per_block]"""
        if t.dtype == self.torch.uint16:
            return t.view(self.torch.int16).view(N, per_block)[self.d_picks].cpu().numpy().view(np.uint16)
        return t.view(N, per_block)[self.d_picks].cpu().numpy()

    # ---- torch's side ----
    def chunks(self):
        return [(b0, min(b0 + CHUNK, N)) for b0 in range(0, N, CHUNK)]

    def bits(self, words, b0, b1):
        """bool[b1 - b0, 1024] of the mask words of the blocks b0 .. b1 - 1"""
        torch = self.torch
        shifts = torch.arange(32, dtype=torch.int32, device=words.device)
        return ((words.view(N, 32, 1)[b0:b1] >> shifts) & 1).bool().view(b1 - b0, 1024)

    def rows(self, v, b0, b1):
        """int64[b1 - b0, 1024] of a decoded column (u8, or u16 through its int16 view)"""
        torch = self.torch
        if v.dtype == torch.uint8:
            return v.view(N, 1024)[b0:b1].to(torch.int64)
        return v.view(torch.int16).view(N, 1024)[b0:b1].to(torch.int64) & 0xFFFF

    def popcounts(self, words):
        torch = self.torch
        by = words.view(N, 32).view(torch.uint8).view(N, 128)
        pop = torch.zeros(N, dtype=torch.int64, device=words.device)
        for bit in range(8):
            pop += ((by >> bit) & 1).sum(dim=1)
        return pop

    def slots(self, value_rows, masked):
        """int64[N, 4] = count, sum, min, max of every block over value_rows(b0, b1) (int64 rows) under the mask (or every row)"""
        torch = self.torch
        out = torch.empty((N, 4), dtype=torch.int64, device="cuda:0")
        for b0, b1 in self.chunks():
            v = value_rows(b0, b1)
            if masked:
                k = self.bits(self.words, b0, b1)
                count = k.sum(dim=1)
                out[b0:b1, 0], out[b0:b1, 1] = count, (v * k).sum(dim=1)
                out[b0:b1, 2] = torch.where(count > 0, torch.where(k, v, BIG).amin(dim=1), I64_MINUS_1)
                out[b0:b1, 3] = torch.where(k, v, 0).amax(dim=1)
            else:
                out[b0:b1, 0], out[b0:b1, 1], out[b0:b1, 2], out[b0:b1, 3] = 1024, v.sum(dim=1), v.amin(dim=1), v.amax(dim=1)
        return out

    def groups(self, code_rows, value_rows, masked, present):
        """int64[256, 4] over the rows the mask keeps (or every row), grouped by code_rows(b0, b1) (int64 rows, every code one of
        `present`): the rows of every other group hold the identity"""
        torch = self.torch
        out = torch.tensor([[0, 0, BIG, 0]] * 256, dtype=torch.int64, device="cuda:0")
        allowed = torch.zeros(256, dtype=torch.bool, device="cuda:0")
        allowed[torch.tensor(sorted(present), device="cuda:0")] = True
        for b0, b1 in self.chunks():
            code, v = code_rows(b0, b1), value_rows(b0, b1)
            assert bool(allowed[code].all())
            k = self.bits(self.words, b0, b1) if masked else None
            for g in present:
                sel = (code == g) if k is None else (code == g) & k
                out[g, 0] += sel.sum()
                out[g, 1] += (v * sel).sum()
                out[g, 2] = torch.minimum(out[g, 2], torch.where(sel, v, BIG).amin())
                out[g, 3] = torch.maximum(out[g, 3], torch.where(sel, v, 0).amax())
        out[:, 2] = torch.where(out[:, 0] > 0, out[:, 2], I64_MINUS_1)
        return out

    def combined(self, slots):
        torch = self.torch
        mins = slots[:, 2]
        kept = mins[slots[:, 0] > 0]
        return torch.stack([slots[:, 0].sum(), slots[:, 1].sum(), kept.amin() if kept.numel() else torch.tensor(I64_MINUS_1, device="cuda:0"),
                            slots[:, 3].amax()])


@pytest.fixture(scope="module")
def col(fl):
    import torch
    c = Column(fl)
    yield c
    del c
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def free_cached_memory():
    yield
    import torch
    torch.cuda.empty_cache()


def sentinel_slots():
    import torch
    buf = torch.full(((N + GUARD) * 4,), int(SENTINEL.view(np.int64)), dtype=torch.int64, device="cuda:0")
    return buf, buf[:N * 4]


def sample_slots(col, vals_s, masked):
    return gs.expected_blocks(vals_s.reshape(-1), col.keep_s.reshape(-1) if masked else None)


def test_the_kept_count_passes_2_32_inside_the_column(col):
    assert ROWS > 1 << 32 and col.kept > 1 << 32, (ROWS, col.kept)
    assert abs(col.kept - ROWS * (1 - 1 / 128)) < ROWS * 1e-4
    assert 0 < col.cross < N - 1000 and col.oo_np[col.cross] <= 1 << 32 < col.oo_np[col.cross + 1]
    assert {0, N - 1, (1 << 22) - 1, 1 << 22, col.cross} <= set(col.picks.tolist()) and (col.picks % 64 == 0).sum() >= 30


def test_mask_offsets(fl, col):
    import torch
    oo, total = fl.mask_offsets(col.words)
    assert torch.equal(oo, torch.cumsum(col.pop, 0) - col.pop)
    assert int(total.item()) == col.kept > 1 << 32
    assert np.array_equal(oo.cpu().numpy(), col.oo_np)


@pytest.mark.parametrize("which", ["unfor_select", "undelta_select"])
def test_select(fl, col, which):
    """the whole output equals masked_select of the decoded column; the guard behind `total` is untouched"""
    import torch
    vals, vals_s = (col.decoded("a"), col.a_s) if which == "unfor_select" else (col.decoded("delta"), col.d_s)
    oo, total = fl.mask_offsets(col.words)
    out = torch.full((col.kept + GUARD,), int(gs.sentinel_of("u8")), dtype=torch.uint8, device="cuda:0")
    if which == "unfor_select":
        got = fl.FoR.unfor_select(1, col.pk, col.refs, col.words, out_offsets=oo, total=total, output=out)
    else:
        got = fl.Delta.undelta_select(1, col.pk, col.bases, col.words, out_offsets=oo, total=total, output=out)
    assert got.data_ptr() == out.data_ptr()
    for b0, b1 in col.chunks():
        want = vals.view(N, 1024)[b0:b1][col.bits(col.words, b0, b1)]
        o0 = int(col.oo_np[b0])
        assert want.numel() == int(col.pop_np[b0:b1].sum())
        assert torch.equal(out[o0:o0 + want.numel()], want), (which, "blocks", b0, b1)
    assert bool((out[col.kept:] == int(gs.sentinel_of("u8"))).all()), (which, "the guard was written")
    for j, b in enumerate(col.picks):                                           # the sampled runs against the oracle
        run = out[int(col.oo_np[b]):int(col.oo_np[b]) + int(col.pop_np[b])].cpu().numpy()
        assert np.array_equal(run, vals_s[j][col.keep_s[j]]), (which, int(b))


AGGREGATES = {
    "unfor_aggregate": (("a",), lambda fl, c, m, s: fl.FoR.unfor_aggregate(1, c.pk, c.refs, mask=m, block_aggs=s)),
    "undelta_aggregate": (("delta",), lambda fl, c, m, s: fl.Delta.undelta_aggregate(1, c.pk, c.bases, mask=m, block_aggs=s)),
    "unfor_aggregate_columns": (("a", "b"), lambda fl, c, m, s: fl.FoR.unfor_aggregate_columns(1, c.pk, c.refs, "*", 1, c.pk_b, c.refs_b, mask=m, block_aggs=s)),
}


@pytest.mark.parametrize("which", list(AGGREGATES))
def test_aggregate(fl, col, which):
    """all N slots, with no mask (count = N * 1024 > 2^32) and under the mask"""
    import torch
    cols, call = AGGREGATES[which]
    decoded = [col.decoded(w) for w in cols]
    sample = {"a": col.a_s, "b": col.b_s, "delta": col.d_s}
    value_rows = (lambda b0, b1: col.rows(decoded[0], b0, b1) * col.rows(decoded[1], b0, b1)) if len(cols) == 2 else (lambda b0, b1: col.rows(decoded[0], b0, b1))
    vals_s = sample[cols[0]].astype(np.uint64) * sample[cols[1]].astype(np.uint64) if len(cols) == 2 else sample[cols[0]]
    for masked in (False, True):
        buf, slots = sentinel_slots()
        result, _ = call(fl, col, col.words if masked else None, slots)
        want = col.slots(value_rows, masked)
        assert torch.equal(slots.view(N, 4), want), (which, masked)
        assert bool((buf[N * 4:] == int(SENTINEL.view(np.int64))).all()), (which, "the guard was written")
        assert torch.equal(result, col.combined(want)), (which, masked, result, col.combined(want))
        assert int(result[0].item()) == (col.kept if masked else ROWS) > 1 << 32
        assert np.array_equal(col.sample(slots, 4).view(np.uint64), sample_slots(col, vals_s, masked)), (which, masked, "the sampled slots against the oracle")
        del buf, slots, want
    col.drop("b")


GROUPED = {
    "unfor_aggregate_by": lambda fl, c, m, kw, kpk, kref: fl.FoR.unfor_aggregate_by(1, c.pk, c.refs, kw, kpk, kref, mask=m, n_blocks=N),
    "unfor_aggregate_by_columns": lambda fl, c, m, kw, kpk, kref: fl.FoR.unfor_aggregate_by_columns(1, c.pk, c.refs, "*", 1, c.pk_b, c.refs_b, kw, kpk, kref,
                                                                                                   mask=m, n_blocks=N),
    "unfor_aggregate_by_lookup": lambda fl, c, m, kw, kpk, kref: fl.FoR.unfor_aggregate_by_lookup(1, c.pk, c.refs, kw, kpk, kref, 0, c.code_table, mask=m,
                                                                                                 n_blocks=N)[0],
}


@pytest.mark.parametrize("which", list(GROUPED))
def test_grouped_aggregate(fl, col, which):
    """a width-0 key column with one constant key: one group with count > 2^32 (no mask: N * 1024), every other group the identity;
    then a W = 1 key column (keys 0 .. 5) under the mask"""
    import torch
    a = col.decoded("a")
    if which == "unfor_aggregate_by_columns":
        b = col.decoded("b")
        value_rows = lambda b0, b1: col.rows(a, b0, b1) * col.rows(b, b0, b1)
    else:
        value_rows = lambda b0, b1: col.rows(a, b0, b1)
    table = np.random.default_rng(9102).permutation(256).astype(np.uint8)          # the lookup's group codes: a permutation of the keys
    col.code_table = to_dev(table)
    code_of = (lambda k: int(table[k])) if which == "unfor_aggregate_by_lookup" else (lambda k: k)
    empty = torch.empty(0, dtype=torch.uint8, device="cuda:0")
    for masked in (False, True):
        got = GROUPED[which](fl, col, col.words if masked else None, 0, empty, 7)
        g = code_of(7)
        want = col.groups(lambda b0, b1: torch.full((b1 - b0, 1024), g, dtype=torch.int64, device="cuda:0"), value_rows, masked, [g])
        assert torch.equal(got, want), (which, "constant key", masked, got[g], want[g])
        assert int(got[g, 0].item()) == (col.kept if masked else ROWS) > 1 << 32
        assert int((got[:, 0] != 0).sum().item()) == 1
    keys = col.decoded("key")
    lut = torch.from_numpy(table.astype(np.int64)).cuda() if which == "unfor_aggregate_by_lookup" else torch.arange(256, device="cuda:0")
    got = GROUPED[which](fl, col, col.words, 1, col.pk_b, col.key_refs)
    want = col.groups(lambda b0, b1: lut[col.rows(keys, b0, b1)], value_rows, True, [code_of(k) for k in range(6)])
    assert torch.equal(got, want), (which, "W = 1 key")
    assert int(got[:, 0].sum().item()) == col.kept
    col.drop("b", "key")


@pytest.mark.parametrize("tier", ["LDS", "device atomics"])
def test_aggregate_by_window_one_slot_passes_2_32(fl, col, tier):
    """a width-0 key column whose constant key is slot 7 of the window: that slot's count is the kept count > 2^32 (no mask: N * 1024),
    stats inside the same.  The LDS tier in u8 with 200 groups; above 256 groups a u8 key has no window, so the device-atomic tier runs
    the same packed bytes as a u16 column (W = 1: 64 u16 per block) with 300 groups."""
    import torch
    if tier == "LDS":
        pk, refs, lo, ng, vals, vals_s = col.pk, col.refs, 30, 200, col.decoded("a"), col.a_s
    else:
        refs_np = ((np.arange(N) % 200) * 300).astype(np.uint16)
        pk, refs, lo, ng = col.pk.view(torch.uint16), to_dev(refs_np), 40000, 300
        vals = fl.FoR.unfor_pack(1, pk, refs)
        o = load_oracle()
        vals_s = np.stack([o.unfor_pack("u16", 1, col.pk_s[j].view(np.uint16), int(refs_np[b])) for j, b in enumerate(col.picks)])
        assert np.array_equal(col.sample(vals, 1024), vals_s)
    empty = torch.empty(0, dtype=pk.dtype, device="cuda:0")
    for masked in (False, True):
        table, stats = fl.FoR.unfor_aggregate_by_window(1, pk, refs, 0, empty, lo + 7, lo, ng, mask=col.words if masked else None,
                                                        what=("count", "sum", "min", "max"), n_blocks=N)
        slots = col.slots(lambda b0, b1: col.rows(vals, b0, b1), masked)
        want = col.combined(slots)
        count = col.kept if masked else ROWS
        assert int(want[0].item()) == count > 1 << 32
        got = torch.stack([t[7] for t in (table.counts, table.sums, table.mins, table.maxs)])
        assert torch.equal(got, want), (tier, masked, got, want)
        for t, identity in ((table.counts, 0), (table.sums, 0), (table.mins, -1), (table.maxs, 0)):
            rest = torch.cat([t[:7], t[8:]])
            assert t.numel() == ng and bool((rest == identity).all()), (tier, masked)
        assert stats.tolist() == [count, 0], (tier, masked, stats)
        del slots


def test_lookup_every_row_and_hit_word(fl, col):
    """the u8 output and the hit mask of every block; stats hits > 2^32"""
    import torch
    keys = col.decoded("a")
    table_np = lkd_table()
    table, missing = to_dev(table_np), 0xEE
    out = torch.full((ROWS + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    hit = torch.full((N * 32 + GUARD,), 0x3C3C3C3C, dtype=torch.int32, device="cuda:0")
    column, h, stats = fl.FoR.unfor_lookup(1, col.pk, col.refs, 0, table, missing=missing, mask=col.words, hit=hit[:N * 32], output=out[:ROWS])
    lut = torch.cat([table, torch.full((256 - SLOTS,), missing, dtype=torch.uint8, device="cuda:0")])
    hits = 0
    for b0, b1 in col.chunks():
        k, keep = col.rows(keys, b0, b1), col.bits(col.words, b0, b1)
        is_hit = keep & (k < SLOTS)
        want = torch.where(is_hit, lut[k], missing).to(torch.uint8)
        assert torch.equal(out[:ROWS].view(N, 1024)[b0:b1], want), ("column", b0, b1)
        assert torch.equal(col.bits(hit[:N * 32], b0, b1), is_hit), ("hit", b0, b1)
        hits += int(is_hit.sum().item())
    assert bool((out[ROWS:] == 0x5A).all()) and bool((hit[N * 32:] == 0x3C3C3C3C).all()), "a guard was written"
    assert stats.tolist() == [hits, col.kept - hits] and hits > 1 << 32, (stats, hits)
    # the sampled blocks against the definition over the oracle's keys
    is_hit = col.keep_s & (col.a_s < SLOTS)
    want = np.where(is_hit, table_np[np.minimum(col.a_s, SLOTS - 1)], missing).astype(np.uint8)
    assert np.array_equal(col.sample(out[:ROWS], 1024), want)
    assert np.array_equal(col.sample(hit[:N * 32], 32).view(np.int32), np.packbits(is_hit, axis=1, bitorder="little").view(np.int32))


def lkd_table():
    import lookup_data
    return lookup_data.table_of("u8", SLOTS, 9103)


def test_set_build_counts_pass_2_32(fl, col):
    """stats inside > 2^32; the set is bit exact"""
    import torch
    vals = col.decoded("a")
    ms, stats = fl.FoR.unfor_set_build(1, col.pk, col.refs, 0, SLOTS, mask=col.words)
    seen = torch.zeros(257, dtype=torch.bool, device="cuda:0")
    inside = 0
    for b0, b1 in col.chunks():
        v, keep = col.rows(vals, b0, b1), col.bits(col.words, b0, b1)
        seen[torch.where(keep, v, 256).view(-1)] = True
        inside += int((keep & (v < SLOTS)).sum().item())
    assert stats.tolist() == [inside, col.kept - inside] and inside > 1 << 32, (stats, inside)
    want = np.packbits(np.concatenate([seen[:SLOTS].cpu().numpy(), np.zeros(-SLOTS % 32, bool)]), bitorder="little").view(np.int32)
    assert np.array_equal(ms.words.cpu().numpy(), want)
    assert want.view(np.uint32).sum() > 0


def _range_hits(col, vals):
    return lambda b0, b1: (lambda v: (v >= LO) & (v <= HI))(col.rows(vals, b0, b1))


COMPARES = {
    "unfor_compare_range": (("a",), lambda fl, c, m: fl.FoR.unfor_compare_range(1, c.pk, c.refs, LO, HI, mask=m, combine="and", output=m),
                            lambda c, v: _range_hits(c, v[0]), lambda c, w: rng_.want_mask(c.a_s.reshape(-1), LO, HI, "and", w)),
    "unfor_compare_in": (("a",), lambda fl, c, m: fl.FoR.unfor_compare_in(1, c.pk, c.refs, MEMBERS, mask=m, combine="and", output=m),
                         lambda c, v: (lambda b0, b1: c.member_lut[c.rows(v[0], b0, b1)]),
                         lambda c, w: cin.want_in(c.a_s.reshape(-1), np.array(MEMBERS, np.uint8), False, "and", w)),
    "unfor_compare_columns": (("a", "b"), lambda fl, c, m: fl.FoR.unfor_compare_columns(1, c.pk, c.refs, "<", 1, c.pk_b, c.refs_b, mask=m, combine="and", output=m),
                              lambda c, v: (lambda b0, b1: c.rows(v[0], b0, b1) < c.rows(v[1], b0, b1)),
                              lambda c, w: columns_data.want_mask(c.a_s.reshape(-1), c.b_s.reshape(-1), "<", False, "and", w)),
    "undelta_compare_range": (("delta",), lambda fl, c, m: fl.Delta.undelta_compare_range(1, c.pk, c.bases, LO, HI, mask=m, combine="and", output=m),
                              lambda c, v: _range_hits(c, v[0]), lambda c, w: dd.want_mask(c.d_s.reshape(-1), LO, HI, "and", w)),
}


@pytest.mark.parametrize("which", list(COMPARES))
def test_compare_in_place_under_the_mask(fl, col, which):
    """combine="and" in place: the masks of all blocks through their popcounts, the sampled blocks word for word"""
    import torch
    cols, call, hits_of, sample_want = COMPARES[which]
    col.member_lut = torch.zeros(256, dtype=torch.bool, device="cuda:0")
    col.member_lut[torch.tensor(MEMBERS, device="cuda:0")] = True
    decoded = [col.decoded(w) for w in cols]
    m = col.words.clone()
    got = call(fl, col, m)
    assert got.data_ptr() == m.data_ptr()
    hits = hits_of(col, decoded)
    want_pop = torch.empty(N, dtype=torch.int64, device="cuda:0")
    for b0, b1 in col.chunks():
        want_pop[b0:b1] = (hits(b0, b1) & col.bits(col.words, b0, b1)).sum(dim=1)
    assert torch.equal(col.popcounts(m), want_pop), which
    assert 0 < int(want_pop.sum().item()) < col.kept
    assert np.array_equal(col.sample(m, 32).view(np.int32).reshape(-1), sample_want(col, col.words_s.reshape(-1))), (which, "the sampled blocks")
    col.drop("b")
