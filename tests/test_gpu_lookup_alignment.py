"""GPU: unfor_lookup / unfor_lookup_widths and their uint8-payload twins with every pointer argument at a merely-16-byte-aligned
address inside a larger buffer, after the pattern of tests/test_gpu_alignment.py (the padded mixed-width column whose blocks start on
every 16-byte residue, the uniform column, placed buffers with guard bytes): the packed column at both bases, widths / offsets /
references / mask / table / present / err_flag at residues of their own, and the three buffers the call WRITES THROUGH -- out, hit_mask
and stats -- at 16-byte offsets as well, in the LDS tier (40 slots) and in the memory tier (one slot above the boundary).  Every
result is compared bit for bit with the model of tests/lookup_data.py; after every call every byte outside every payload must be what
it was."""
import numpy as np
import pytest

import gpu_support as gs
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import placed
from lookup_data import PAIRS, RUN_OF_3, STATS_PREFILL, boundary_slots, entry, expected_lookup, present_words, table_of
from oracle_lib import load_oracle, tbits
from test_gpu_alignment import cabi, column_case, flag_clear, guards, same, seeds_from, zero_flag
from test_gpu_for_consumer_shapes import column_masks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("policy", [0, RUN_OF_3], ids=["one block per wavefront", "runs of 3"])
@pytest.mark.parametrize("ty,uty", PAIRS, ids=[f"{t}-{u}" for t, u in PAIRS])
def test_lookup_off_the_128_byte_boundary(fl, kernel_policy, ty, uty, policy):
    kernel_policy(policy)
    n = gs.aligned_column_blocks(1)
    T, esz, U = tbits(ty), tbits(ty) // 8, tbits(uty)
    N = 1 << T
    oracle = load_oracle()
    c = column_case(ty, n)
    seed = seeds_from(82000 + 1000 * T + 10 * U + (policy != 0))
    wu = T // 2 + 1
    pku = gs.uniform_packed(ty, wu, n)
    valsu = oracle.batch("unfor_pack", ty, wu, pku, aux=c["refs"], n_blocks=n)
    keep, words = column_masks(n, 82300 + n)
    narrow = int(np.argmin(np.where(c["widths"] >= 2, c["widths"], 99)))               # the narrowest block: a small window holds its keys
    lo = (int(c["refs"][narrow]) - 3) % N
    windows = [(lo, 40)] + ([((lo - 1000) % N, boundary_slots(ty, uty) + 1)] if T > 8 else [])
    for base in gs.ALIGNED_COLUMN_BASES:
        k = base // 16
        d_col, d_pku = placed(c["col"], ty, base, gs.column_seed(ty, n, base)), placed(pku, ty, base, gs.packed_seed(ty, wu, base))
        d_w, d_off = placed(c["widths"], "uint8", 16 * (k + 1), seed()), placed(c["off"], "int64", 16 * (8 - k), seed())
        d_refs = placed(c["refs"], ty, esz, seed())
        d_m = placed(words, "int32", 16, seed())
        for q, (wlo, slots) in enumerate(windows):
            table, pw = table_of(uty, slots, 82400 + slots % 1000), present_words(slots, 82500 + q)
            d_tb = placed(table, uty, 16 * (1 + (k + q) % 7), seed())
            d_pr = placed(pw.view(np.int32), "int32", 16 * (1 + (k + 3 * q) % 7), seed())
            for form, vals, ins in (("mixed", c["unfor_pack"], (d_col, d_w, d_off, d_refs)), ("uniform", valsu, (d_pku, d_refs))):
                for j, (mask, kept, present) in enumerate(((d_m, keep, d_pr), (None, None, None))):
                    what = (ty, uty, policy, n, base, form, slots, "mask" if mask else "no mask")
                    d_out = placed(n * 1024 * (U // 8), uty, 16 * (1 + (k + 2 * q + j) % 7), seed())
                    d_hit = placed(n * 128, "int32", 16 * (1 + (k + q + 2 * j) % 7), seed())
                    d_st = placed(STATS_PREFILL.view(np.int64), "int64", 16 * (1 + (k + q + 3 * j) % 7), seed())
                    for p in (d_out, d_hit, d_st, d_tb, d_pr):
                        assert p.t.data_ptr() % 128 and p.t.data_ptr() % 16 == 0
                    tail = (mask.t.data_ptr() if mask else None, n, wlo, slots, d_tb.t.data_ptr(), present.t.data_ptr() if present else None, 3,
                            d_out.t.data_ptr(), d_hit.t.data_ptr(), d_st.t.data_ptr())
                    if form == "mixed":
                        flag = zero_flag(seed())
                        cabi(fl, entry(ty, uty, True), d_w.t.data_ptr(), d_off.t.data_ptr(), d_col.t.data_ptr(), d_col.nbytes, d_refs.t.data_ptr(), 1,
                             *tail, flag.t.data_ptr())
                        flag_clear(flag, what)
                        flag.check_guards(what)
                    else:
                        cabi(fl, entry(ty, uty, False), wu, d_pku.t.data_ptr(), d_refs.t.data_ptr(), 1, *tail)
                    want = expected_lookup(oracle, ty, uty, vals, kept, wlo, table, pw if present else None, 3, STATS_PREFILL)
                    if form == "mixed" and q == 0 and kept is None:
                        assert want[2][0] > STATS_PREFILL[0], what
                    same(d_out, want[0], what)
                    same(d_hit, want[1], what)
                    same(d_st, want[2], what)
                    guards(what, d_out, d_hit, d_st, d_m, d_tb, d_pr, *ins)
