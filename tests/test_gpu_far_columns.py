"""GPU: every mixed-width entry point of the Python mirror on a FAR column -- two dozen blocks scattered over one packed buffer of
2^33 + 2^20 bytes (tests/far_column_data.py; tests/test_far_column_data_cpu.py pins it), so that offsets[b] needs bit 31, bit 32 and
bit 33, is not ascending, and a kernel that drops, swaps or sign-extends a half of the offset, or forms a byte or element address in
32 bits, reads a decoy, another block or noise.  The buffer is allocated once per element type and variant, filled with
fl_fill_random (a stray read yields noise, not zeros), then the blocks and decoys are written.  Two- and three-column calls take all
their columns from the SAME buffer.

Every result is compared bit for bit, in sentinel-filled outputs, with the existing definitions over the oracle's decode of the blocks
(gpu_support.want_mask / expected_blocks, the *_data.py modules), and must equal the same call on the compact copy of the same blocks
(offsets = the exclusive prefix sum of 128 * W, in a small buffer).  Each call runs under the default kernel policy and under
gpu_support.POLICIES[3] (several blocks per wavefront: the offset is broadcast from a lane, not from the first one), without a mask
and -- wherever the call takes one -- under a random incoming mask.  The three encoders write AT the far offsets: the blocks are read
back, and nothing else may have moved.  The device checks keep working up there: a block that passes packed_bytes by 16 bytes is
skipped and flagged alone, an offset of 2^33 + 8 is flagged as misaligned."""
import ctypes

import numpy as np
import pytest

import aggregate_by_lookup_data as abl
import aggregate_by_window_data as abw
import columns_data
import delta_aggregate_data as dad
import delta_compare_range_data as dd
import delta_select_data as dsd
import far_column_data as fcd
import group_columns_data as gcd
import group_data
import gpu_support as gs
import lookup_data as lkd
import set_build_data as sbd
import test_gpu_for_compare_in as cin
import test_gpu_for_compare_range as rng_
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import GUARD, IDENTITY, POLICIES, SENTINEL, TDT, TYS, to_dev
from oracle_lib import TYPES, load_oracle, tbits

pytestmark = pytest.mark.gpu

RUNS = POLICIES[3]                              # wave-per-block kernels, 4 blocks per wavefront
N = fcd.N_BLOCKS
NEAR = 4096                                     # bytes in front of and behind every block that an encoder must leave alone


def far_masks(a, seed):
    """bool[N * 1024] at half density and the same as int32 words; the plain width-1 block's mask is empty, the mask of the named block
    above 2^33 is full"""
    bits = np.random.default_rng(seed).random(a.n * 1024) < 0.5
    empty, full = (int(np.flatnonzero(a.off == off)[0]) for off in (3 << 20, fcd.B33 + fcd.SLOT + 16))
    bits[empty * 1024:(empty + 1) * 1024] = False
    bits[full * 1024:(full + 1) * 1024] = True
    return bits, np.packbits(bits, bitorder="little").view(np.int32)


# ---- the buffer, once per element type and variant ----
class Dev:
    """a column on the device: widths, offsets, the packed tensor they index, references and bases"""

    def __init__(self, c, pk, off):
        self.c, self.ty, self.n, self.pk = c, c.ty, c.n, pk
        self.w, self.off, self.refs, self.bases = to_dev(c.widths), to_dev(off), to_dev(c.refs), to_dev(c.bases)


class Far:
    def __init__(self, fl, ty, variant):
        import torch
        self.ty, self.variant, self.fb = ty, variant, fcd.far_buffer(ty, variant)
        self.buf = torch.empty(fcd.PACKED_BYTES // (tbits(ty) // 8), dtype=getattr(torch, TDT[ty]), device="cuda:0")
        self.u8 = self.buf.view(torch.uint8)
        assert self.u8.numel() == fcd.PACKED_BYTES
        rc = fl.load().fl_fill_random(self.buf.data_ptr(), fcd.PACKED_BYTES, 4100 + tbits(ty), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, (rc, fl.load().fl_last_hip_error())
        for off, r in self.fb.regions.items():
            self.u8[off:off + len(r)] = to_dev(r)
        cols = self.fb.columns
        self.far = {role: Dev(c, self.u8 if c.ty == "u8" else self.buf, c.off) for role, c in cols.items()}
        self.compact = {role: Dev(c, to_dev(c.compact), c.compact_off) for role, c in cols.items()}
        self.keep, self.words = far_masks(cols["a"], 4200 + tbits(ty))
        self.mask = to_dev(self.words)
        torch.cuda.synchronize()

    def checksum(self):
        """the wrapping int64 sum of the whole buffer"""
        import torch
        return int(self.u8.view(torch.int64).sum().item())


@pytest.fixture(scope="module", params=[(ty, v) for ty in TYS for v in fcd.VARIANTS], ids=lambda p: f"{p[0]}-{p[1]}")
def far(request, fl):
    import torch
    f = Far(fl, *request.param)
    before = f.checksum()
    yield f
    assert f.checksum() == before, "a test left the far buffer changed"
    del f
    torch.cuda.empty_cache()


class Outs:
    """sentinel-filled outputs with GUARD sentinel elements behind each"""

    def __init__(self):
        self.made = []

    def new(self, kind, n, fill=None):
        """a tensor of n elements of an element type of TYS or of "int32" / "int64"; fill: the payload's initial words (a mask in place)"""
        import torch
        dt = np.dtype(TDT.get(kind, kind))
        host = np.full(n + GUARD, SENTINEL.astype(np.dtype(f"u{dt.itemsize}")), dtype=np.dtype(f"u{dt.itemsize}")).view(dt)
        if fill is not None:
            host[:n] = fill
        t = to_dev(host)
        self.made.append((t, n, host[n:].copy()))
        return t[:n]

    def guards(self, what):
        for t, n, want in self.made:
            assert np.array_equal(t[n:].cpu().numpy(), want), (what, "the guard behind an output was written")


def raw(t):
    import torch
    return t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy() if t.numel() else np.zeros(0, np.uint8)


def raw_np(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


# ---- the calls' parameters, from the host image alone ----
def params(F):
    a = F.fb.columns["a"]
    T = tbits(F.ty)
    M = 1 << T
    K = fcd.pivot(F.ty)
    dlo = int(a.undelta_rows[517])
    wlo = (M // 2 + fcd.WINDOW_LO_OFFSET) % M
    return dict(k=K, lo=K, hi=(K + (M >> 2)) % M, dlo=dlo, dhi=(dlo + (M >> 2)) % M,
                members=np.array([(K + d) % M for d in (-4, -2, 0, 1, 3, 5)], dtype=np.uint64).astype(TYPES[F.ty][0]),
                index=np.concatenate([b * 1024 + np.arange(1024) for b in range(N)] + [np.random.default_rng(4300).integers(0, N * 1024, size=257)]).astype(np.int64),
                windows=[(wlo, 40), ((wlo - 100) % M, 300 if T > 8 else 200)])       # the second one holds every key of the cluster's blocks


def combine_of(m):
    return dict(mask=m, combine="and") if m is not None else {}


# ---- entry point -> (does it take a mask, the call, the expected values) ----
# call(fl, F, C, m, O, P): C role -> Dev (far or compact), m the mask on the device or None, O the outputs, P params(F); returns
# label -> tensor.  want(F, keep, words, P): label -> numpy, from the oracle's decode.
def col(F, role):
    return F.fb.columns[role]


def c_unpack(fl, F, C, m, O, P):
    a = C["a"]
    return {"values": fl.unpack_widths(a.w, a.off, a.pk, output=O.new(a.ty, N * 1024))}


def c_unfor_pack(fl, F, C, m, O, P):
    a = C["a"]
    return {"values": fl.unfor_pack_widths(a.w, a.off, a.pk, a.refs, output=O.new(a.ty, N * 1024))}


def c_undelta_pack(fl, F, C, m, O, P):
    a = C["a"]
    return {"transposed": fl.undelta_pack_widths(a.w, a.off, a.pk, a.bases, output=O.new(a.ty, N * 1024)),
            "rows": fl.undelta_pack_widths(a.w, a.off, a.pk, a.bases, output=O.new(a.ty, N * 1024), untranspose=True)}


def c_unpack_single(fl, F, C, m, O, P):
    a = C["a"]
    return {"values": fl.unpack_single_widths(a.w, a.off, a.pk, to_dev(P["index"]))}


def c_compare(fl, F, C, m, O, P):
    a = C["a"]
    return {"mask": fl.unfor_compare_widths(a.w, a.off, a.pk, a.refs, "<", P["k"], output=O.new("int32", N * 32))}


def c_compare_range(fl, F, C, m, O, P):
    a = C["a"]
    out = {"mask": fl.unfor_compare_range_widths(a.w, a.off, a.pk, a.refs, P["lo"], P["hi"], output=O.new("int32", N * 32), **combine_of(m))}
    if m is not None:
        io = O.new("int32", N * 32, fill=F.words)
        out["in place"] = fl.unfor_compare_range_widths(a.w, a.off, a.pk, a.refs, P["lo"], P["hi"], mask=io, combine="and", output=io)
    return out


def c_compare_in(fl, F, C, m, O, P):
    a = C["a"]
    return {"mask": fl.unfor_compare_in_widths(a.w, a.off, a.pk, a.refs, P["members"], output=O.new("int32", N * 32), **combine_of(m))}


def c_compare_columns(fl, F, C, m, O, P):
    a, b = C["a"], C["b"]
    return {"mask": fl.unfor_compare_columns_widths(a.w, a.off, a.pk, a.refs, "<", b.w, b.off, b.pk, b.refs, output=O.new("int32", N * 32),
                                                    **combine_of(m))}


def c_select(fl, F, C, m, O, P):
    a = C["a"]
    oo, total = fl.mask_offsets(m)
    return {"run": fl.unfor_select_widths(a.w, a.off, a.pk, a.refs, m, out_offsets=oo, total=total, output=O.new(a.ty, int(F.keep.sum()))),
            "total": total}


def c_aggregate(fl, F, C, m, O, P):
    a = C["a"]
    slots = O.new("int64", N * 4)
    result, _ = fl.unfor_aggregate_widths(a.w, a.off, a.pk, a.refs, mask=m, block_aggs=slots)
    return {"slots": slots, "result": result}


def c_aggregate_columns(fl, F, C, m, O, P):
    a, b = C["a"], C["b"]
    slots = O.new("int64", N * 4)
    result, _ = fl.unfor_aggregate_columns_widths(a.w, a.off, a.pk, a.refs, "*", b.w, b.off, b.pk, b.refs, mask=m, block_aggs=slots)
    return {"slots": slots, "result": result}


def c_aggregate_by(fl, F, C, m, O, P):
    a, k = C["a"], C["key8"]
    return {"groups": fl.unfor_aggregate_by_widths(a.w, a.off, a.pk, a.refs, k.w, k.off, k.pk, k.refs, mask=m, result=O.new("int64", 256 * 4))}


def c_aggregate_by_columns(fl, F, C, m, O, P):
    a, b, k = C["a"], C["b"], C["key8"]
    return {"groups": fl.unfor_aggregate_by_columns_widths(a.w, a.off, a.pk, a.refs, "+", b.w, b.off, b.pk, b.refs, k.w, k.off, k.pk, k.refs, mask=m,
                                                           result=O.new("int64", 256 * 4))}


def c_aggregate_by_window(fl, F, C, m, O, P):
    a, k = C["a"], C["key"]
    out = {}
    for lo, ng in P["windows"]:
        table, stats = fl.unfor_aggregate_by_window_widths(a.w, a.off, a.pk, a.refs, k.w, k.off, k.pk, k.refs, lo, ng, mask=m,
                                                           what=("count", "sum", "min", "max"))
        out.update({f"{name} {ng}": t for name, t in zip(abw.WHAT, (table.counts, table.sums, table.mins, table.maxs))})
        out[f"stats {ng}"] = stats
    return out


def present_of(fl, F, lo, slots):
    return fl.MemberSet(F.ty, lo, slots, lkd.present_words(slots, 4400 + slots))


def c_aggregate_by_lookup(fl, F, C, m, O, P):
    a, k = C["a"], C["key"]
    out = {}
    for lo, slots in P["windows"]:
        present = present_of(fl, F, lo, slots) if m is not None else None
        groups, stats = fl.unfor_aggregate_by_lookup_widths(a.w, a.off, a.pk, a.refs, k.w, k.off, k.pk, k.refs, lo, to_dev(abl.code_table(slots, 4500 + slots)),
                                                            present=present, mask=m, result=O.new("int64", 256 * 4))
        out[f"groups {slots}"], out[f"stats {slots}"] = groups, stats
    return out


def c_set_build(fl, F, C, m, O, P):
    s = C["src"]
    out = {}
    for lo, bits in P["windows"]:
        ms, stats = fl.unfor_set_build_widths(s.w, s.off, s.pk, s.refs, lo, bits, mask=m)
        out[f"words {bits}"], out[f"stats {bits}"] = ms.words, stats
    return out


def c_lookup(fl, F, C, m, O, P):
    k = C["key"]
    out = {}
    for lo, slots in P["windows"]:
        present = present_of(fl, F, lo, slots) if m is not None else None
        column, hit, stats = fl.unfor_lookup_widths(k.w, k.off, k.pk, k.refs, lo, to_dev(lkd.table_of(F.ty, slots, 4600 + slots)), present=present,
                                                    missing=(1 << tbits(F.ty)) - 1, mask=m, hit=O.new("int32", N * 32), output=O.new(F.ty, N * 1024))
        out[f"column {slots}"], out[f"hit {slots}"], out[f"stats {slots}"] = column, hit, stats
    return out


def c_delta_compare_range(fl, F, C, m, O, P):
    a = C["a"]
    return {"mask": fl.undelta_compare_range_widths(a.w, a.off, a.pk, a.bases, P["dlo"], P["dhi"], output=O.new("int32", N * 32), **combine_of(m))}


def c_delta_aggregate(fl, F, C, m, O, P):
    a = C["a"]
    slots = O.new("int64", N * 4)
    result, _ = fl.undelta_aggregate_widths(a.w, a.off, a.pk, a.bases, mask=m, block_aggs=slots)
    return {"slots": slots, "result": result}


def c_delta_select(fl, F, C, m, O, P):
    a = C["a"]
    oo, total = fl.mask_offsets(m)
    return {"run": fl.undelta_select_widths(a.w, a.off, a.pk, a.bases, m, out_offsets=oo, total=total, output=O.new(a.ty, int(F.keep.sum()))),
            "total": total}


def slots_and_result(slots):
    return {"slots": slots, "result": gs.combine(slots)}


def w_compare_range(F, keep, words, P):
    want = {"mask": rng_.want_mask(col(F, "a").unfor, P["lo"], P["hi"], "and" if words is not None else "new", words)}
    if words is not None:
        want["in place"] = want["mask"]
    return want


def w_window(F, keep, words, P):
    want = {}
    for lo, ng in P["windows"]:
        arrays, stats = abw.expected_table(F.ty, col(F, "a").unfor, col(F, "key").unfor, keep, lo, ng)
        want.update({f"{name} {ng}": x for name, x in zip(abw.WHAT, arrays)})
        want[f"stats {ng}"] = stats
    return want


def w_by_lookup(F, keep, words, P):
    want = {}
    for lo, slots in P["windows"]:
        present = lkd.present_words(slots, 4400 + slots) if keep is not None else None
        want[f"groups {slots}"], want[f"stats {slots}"] = abl.expected_fused(F.ty, col(F, "a").unfor, col(F, "key").unfor, keep, lo,
                                                                              abl.code_table(slots, 4500 + slots), present)[:2]
    return want


def w_set_build(F, keep, words, P):
    want = {}
    for lo, bits in P["windows"]:
        want[f"words {bits}"], want[f"stats {bits}"] = sbd.expected_build(F.ty, col(F, "src").unfor, keep, lo, bits)
    return want


def w_lookup(F, keep, words, P):
    want = {}
    for lo, slots in P["windows"]:
        present = lkd.present_words(slots, 4400 + slots) if keep is not None else None
        want[f"column {slots}"], want[f"hit {slots}"], want[f"stats {slots}"] = lkd.expected_lookup(
            load_oracle(), F.ty, F.ty, col(F, "key").unfor, keep, lo, lkd.table_of(F.ty, slots, 4600 + slots), present, (1 << tbits(F.ty)) - 1)[:3]
    return want


def with_mask(words):
    return "and" if words is not None else "new"


ENTRIES = {
    "unpack_widths": (False, c_unpack, lambda F, keep, words, P: {"values": col(F, "a").unpack}),
    "unfor_pack_widths": (False, c_unfor_pack, lambda F, keep, words, P: {"values": col(F, "a").unfor}),
    "undelta_pack_widths": (False, c_undelta_pack, lambda F, keep, words, P: {"transposed": col(F, "a").undelta, "rows": col(F, "a").undelta_rows}),
    "unpack_single_widths": (False, c_unpack_single, lambda F, keep, words, P: {"values": col(F, "a").unpack[P["index"]]}),
    "unfor_compare_widths": (False, c_compare, lambda F, keep, words, P: {"mask": gs.want_mask(col(F, "a").unfor, "<", P["k"])}),
    "unfor_compare_range_widths": (True, c_compare_range, w_compare_range),
    "unfor_compare_in_widths": (True, c_compare_in,
                                lambda F, keep, words, P: {"mask": cin.want_in(col(F, "a").unfor, P["members"], False, with_mask(words), words)}),
    "unfor_compare_columns_widths": (True, c_compare_columns, lambda F, keep, words, P: {
        "mask": columns_data.want_mask(col(F, "a").unfor, col(F, "b").unfor, "<", False, with_mask(words), words)}),
    "unfor_select_widths": ("always", c_select, lambda F, keep, words, P: {"run": col(F, "a").unfor[keep], "total": np.array([keep.sum()], np.int64)}),
    "unfor_aggregate_widths": (True, c_aggregate, lambda F, keep, words, P: slots_and_result(gs.expected_blocks(col(F, "a").unfor, keep))),
    "unfor_aggregate_columns_widths": (True, c_aggregate_columns, lambda F, keep, words, P: slots_and_result(
        gs.expected_blocks(gcd.expr("*", col(F, "a").unfor, col(F, "b").unfor), keep))),
    "unfor_aggregate_by_widths": (True, c_aggregate_by,
                                  lambda F, keep, words, P: {"groups": group_data.expected_groups(col(F, "a").unfor, col(F, "key8").unfor, keep)}),
    "unfor_aggregate_by_columns_widths": (True, c_aggregate_by_columns, lambda F, keep, words, P: {
        "groups": group_data.expected_groups(gcd.expr("+", col(F, "a").unfor, col(F, "b").unfor), col(F, "key8").unfor, keep)}),
    "unfor_aggregate_by_window_widths": (True, c_aggregate_by_window, w_window),
    "unfor_aggregate_by_lookup_widths": (True, c_aggregate_by_lookup, w_by_lookup),
    "unfor_set_build_widths": (True, c_set_build, w_set_build),
    "unfor_lookup_widths": (True, c_lookup, w_lookup),
    "undelta_compare_range_widths": (True, c_delta_compare_range, lambda F, keep, words, P: {
        "mask": dd.want_mask(col(F, "a").undelta_rows, P["dlo"], P["dhi"], with_mask(words), words)}),
    "undelta_aggregate_widths": (True, c_delta_aggregate, lambda F, keep, words, P: slots_and_result(dad.want_slots(col(F, "a").undelta_rows, words))),
    "undelta_select_widths": ("always", c_delta_select, lambda F, keep, words, P: {
        "run": dsd.want_run(col(F, "a").undelta_rows, words)[0], "total": np.array([keep.sum()], np.int64)}),
}
CASES = [(name, policy, masked) for name, (takes, _, _) in ENTRIES.items() for policy in (0, RUNS)
         for masked in ((True,) if takes == "always" else (False, True) if takes else (False,))]


def run(fl, F, name, C, masked):
    _, call, _ = ENTRIES[name]
    O = Outs()
    got = call(fl, F, C, F.mask if masked else None, O, params(F))
    O.guards(name)
    return {label: raw(t) for label, t in got.items()}


@pytest.mark.parametrize("name,policy,masked", CASES, ids=[f"{n}-{'runs' if p else 'default'}-{'mask' if m else 'no mask'}" for n, p, m in CASES])
def test_far_column_equals_the_oracle_and_the_compact_copy(fl, kernel_policy, far, name, policy, masked):
    kernel_policy(policy)
    what = (far.ty, far.variant, name, policy, masked)
    want = ENTRIES[name][2](far, far.keep if masked else None, far.words if masked else None, params(far))
    got = run(fl, far, name, far.far, masked)
    assert set(got) == set(want), what
    for label, w in want.items():
        g, w = got[label], raw_np(w)
        assert g.size == w.size, what + (label, g.size, w.size)
        assert np.array_equal(g, w), what + (label, "first wrong byte", int(np.flatnonzero(g != w)[0]), "of", g.size)
    near = run(fl, far, name, far.compact, masked)
    for label in want:
        assert np.array_equal(got[label], near[label]), what + (label, "differs from the compact copy's")


def test_the_calls_decode_far_blocks(far):
    """No case above can be answered without reading the far blocks: every far block of width > 0 of the primary column has rows that
    satisfy and rows that fail each predicate (so no reference and width decide it), under the mask as well for all but the one block
    whose mask is empty; every far block of the key and set-source columns has values inside the larger window."""
    a = col(far, "a")
    P = params(far)
    far_blocks = [b for b in range(N) if a.cls[b] in fcd.FAR_CLASSES]
    assert {a.cls[b] for b in far_blocks} == set(fcd.FAR_CLASSES) and all(a.widths[b] for b in far_blocks)
    kept = far.keep.reshape(N, 1024)
    assert all(kept[b].any() for b in far_blocks)
    hits = {"compare": gs.CMP["<"](a.unfor, a.unfor.dtype.type(P["k"])), "range": rng_.hit_bits(a.unfor, P["lo"], P["hi"]),
            "in": np.isin(a.unfor, P["members"]), "columns": columns_data.hit_bits(a.unfor, col(far, "b").unfor, "<", False),
            "delta range": dd.hit_bits(a.undelta_rows, P["dlo"], P["dhi"])}
    for name, h in hits.items():
        h = h.reshape(N, 1024)
        for b in far_blocks:
            mixed = 0 < h[b].sum() < 1024 and 0 < (h[b] & kept[b]).sum() < kept[b].sum()
            # (six members among the 2^w values of a wide block may meet none of its 1024 rows: the set's window still lies inside the
            # block's range, which is what keeps the kernel from deciding it)
            excused = {"columns": col(far, "b").widths[b] == 0, "delta range": a.widths[b] < 3, "in": a.widths[b] > 6}.get(name, False)
            assert mixed or excused, (name, b, a.cls[b])
        assert name == "in" or sum(0 < h[b].sum() < 1024 for b in far_blocks) >= len(far_blocks) // 2, name
    lo, slots = P["windows"][-1]
    for role in ("key", "src"):
        c = col(far, role)
        M = 1 << tbits(far.ty)                                                    # the block's slots {(c + f) mod 2^T, f < 2^w} meet the window
        meets = [(int(c.refs[b]) - lo) % M < slots or (int(c.refs[b]) - lo) % M + (1 << int(c.widths[b])) > M for b in range(N)]
        assert all(meets[b] for b in range(N) if c.cls[b] in fcd.FAR_CLASSES), role
        inside = (sbd.window_indices(far.ty, c.unfor, lo) < slots).reshape(N, 1024)
        assert any(inside[b].any() for b in range(N) if c.cls[b] in fcd.FAR_CLASSES), role
    assert sbd.expected_build(far.ty, col(far, "src").unfor, None, *P["windows"][0])[1][0] > 0


# ---- the three encoders write at the far offsets ----
def window_of(off, size):
    return max(off - NEAR, 0), min(off + size + NEAR, fcd.PACKED_BYTES)


@pytest.mark.parametrize("policy", [0, RUNS], ids=["default", "runs"])
@pytest.mark.parametrize("name", ["pack_widths", "for_pack_widths", "transpose_delta_pack_widths"])
def test_encoders_write_the_far_blocks_and_nothing_else(fl, kernel_policy, far, name, policy):
    import torch
    kernel_policy(policy)
    o, ty = load_oracle(), far.ty
    a, d = col(far, "a"), far.far["a"]
    L = 1024 // tbits(ty)
    vals = gs.values(ty, N * 1024, 4700 + tbits(ty))
    block = lambda b: vals[b * 1024:(b + 1) * 1024]
    if name == "pack_widths":
        want = [o.pack(ty, int(w), block(b)) for b, w in enumerate(a.widths)]
        call = lambda dst: fl.pack_widths(dst.w, dst.off, d_vals, dst.pk)
    elif name == "for_pack_widths":
        want = [o.for_pack(ty, int(w), block(b), a.refs[b]) for b, w in enumerate(a.widths)]
        call = lambda dst: fl.for_pack_widths(dst.w, dst.off, d_vals, dst.refs, dst.pk)
    else:
        want = [o.pack(ty, int(w), o.delta(ty, o.transpose(ty, block(b)), a.bases[b * L:(b + 1) * L])) for b, w in enumerate(a.widths)]
        call = lambda dst: fl.transpose_delta_pack_widths(dst.w, dst.off, d_vals, dst.bases, dst.pk)
    d_vals = to_dev(vals)
    what = (ty, far.variant, name, policy)
    held = [(b, int(a.off[b]), int(a.sizes[b])) for b in range(N) if a.widths[b]]
    windows = [window_of(off, size) for _, off, size in held]
    before = [far.u8[s:e].cpu().numpy() for s, e in windows]
    sum_before = far.checksum()
    try:
        call(d)
        torch.cuda.synchronize()
        sum_after = far.checksum()
        # the blocks, and the 4 KiB in front of and behind each (another block of the column may lie there: it holds its new bytes)
        for (b, off, size), (s, e), was in zip(held, windows, before):
            now, expect = far.u8[s:e].cpu().numpy(), was.copy()
            for b2, off2, size2 in held:
                lo, hi = max(off2, s), min(off2 + size2, e)
                if lo < hi:
                    expect[lo - s:hi - s] = want[b2].view(np.uint8)[lo - off2:hi - off2]
            assert np.array_equal(now[off - s:off - s + size], want[b].view(np.uint8)), what + ("block", b, a.cls[b], off)
            assert np.array_equal(now, expect), what + ("bytes near block", b, "at", off, "moved")
        # every decoy, alias source and block of another column
        for off, r in far.fb.regions.items():
            if far.fb.owner[off][0] != "a":
                assert np.array_equal(far.u8[off:off + len(r)].cpu().numpy(), r), what + ("the bytes at", off, far.fb.owner[off], "moved")
        # and the rest of the buffer: its wrapping sum moved by the written blocks' words alone
        delta = sum(int(want[b].view(np.int64).sum(dtype=np.int64)) - int(a.block_bytes(b).view(np.int64).sum(dtype=np.int64)) for b, _, _ in held)
        assert (sum_after - sum_before - delta) % (1 << 64) == 0, what + ("bytes outside the blocks moved",)
    finally:
        for b, off, size in held:
            far.u8[off:off + size] = to_dev(a.block_bytes(b))
        torch.cuda.synchronize()
    assert far.checksum() == sum_before
    # the same call on the compact copy writes the same blocks
    near = far.compact["a"]
    dst = Dev(a, torch.zeros_like(near.pk), a.compact_off)
    call(dst)
    got = raw(dst.pk)
    for b, off, size in held:
        c0 = int(a.compact_off[b])
        assert np.array_equal(got[c0:c0 + size], want[b].view(np.uint8)), what + ("compact block", b)


# ---- the device checks up there ----
def moved(F, b, off):
    offs = col(F, "a").off.copy()
    offs[b] = off
    return to_dev(offs)


@pytest.mark.parametrize("policy", [0, RUNS], ids=["default", "runs"])
def test_a_block_past_the_end_is_skipped_alone_and_a_misaligned_offset_is_flagged(fl, kernel_policy, far, policy):
    """One block of width > 0 moved to packed_bytes - 128 w + 16 (it passes the end by 16 bytes): FL_DEVERR_BOUNDS (bit 8; status 6), and
    only that block is skipped -- its outputs keep the sentinel (an aggregate's slot: the identity), every other block's are the
    oracle's.  The same block at 2^33 + 8: FL_DEVERR_ALIGN (bit 4; status 4), the same block skipped."""
    kernel_policy(policy)
    a, d = col(far, "a"), far.far["a"]
    b = int(np.argmax(a.widths == tbits(far.ty) // 2))
    assert a.widths[b] > 0
    rows = slice(b * 1024, (b + 1) * 1024)
    for off, status in ((fcd.PACKED_BYTES - int(a.sizes[b]) + 16, 6), (fcd.B33 + 8, 4)):
        what = (far.ty, far.variant, policy, b, off)
        d_off = moved(far, b, off)
        O = Outs()
        values, mask, slots, dslots = O.new(far.ty, N * 1024), O.new("int32", N * 32), O.new("int64", N * 4), O.new("int64", N * 4)
        for call in (lambda: fl.unpack_widths(d.w, d_off, d.pk, output=values),
                     lambda: fl.unfor_compare_widths(d.w, d_off, d.pk, d.refs, "<", params(far)["k"], output=mask),
                     lambda: fl.unfor_aggregate_widths(d.w, d_off, d.pk, d.refs, block_aggs=slots),
                     lambda: fl.undelta_aggregate_widths(d.w, d_off, d.pk, d.bases, block_aggs=dslots)):
            with pytest.raises(fl.FastLanesError) as e:
                call()
            assert e.value.status == status, what + (e.value.status,)
        O.guards(what)
        want = a.unpack.copy()
        want[rows] = gs.sentinel_of(far.ty)
        assert np.array_equal(gs.to_np(values, far.ty), want), what + ("unpack_widths",)
        want = gs.want_mask(a.unfor, "<", params(far)["k"]).copy()
        want[b * 32:(b + 1) * 32] = SENTINEL.astype(np.uint32).view(np.int32)
        assert np.array_equal(gs.got_mask(mask), want), what + ("unfor_compare_widths",)
        for got, vals in ((slots, a.unfor), (dslots, a.undelta_rows)):
            want = gs.expected_blocks(vals, None)
            want[b] = IDENTITY
            assert np.array_equal(gs.u64_of(got).reshape(N, 4), want), what + ("aggregate",)
