"""GPU: unfor_aggregate_by_lookup / unfor_aggregate_by_lookup_widths with every pointer argument at a merely-16-byte-aligned address
inside a larger buffer, after the pattern of tests/test_gpu_lookup_alignment.py (the padded mixed-width column whose blocks start on
every 16-byte residue, the uniform column, placed buffers with guard bytes): BOTH packed columns at both bases, widths / offsets /
references of either column, mask, table, present and err_flag at residues of their own, and the two buffers the call WRITES THROUGH
-- result and stats -- at 16-byte offsets as well, with a 40-slot table and one above 8192 slots.  Every result is compared bit for bit
with the model of tests/aggregate_by_lookup_data.py; after every call every byte outside every payload must be what it was."""
import numpy as np
import pytest

import gpu_support as gs
from aggregate_by_lookup_data import FORMS, RUN_OF_3, STATS_PREFILL, code_table, decode, expected_fused, present_words
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import SENTINEL, placed
from oracle_lib import load_oracle, tbits
from test_gpu_alignment import cabi, column_case, flag_clear, guards, same, seeds_from, zero_flag
from test_gpu_for_consumer_shapes import column_masks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("policy", [0, RUN_OF_3], ids=["one block per wavefront", "runs of 3"])
@pytest.mark.parametrize("ty", gs.TYS)
def test_aggregate_by_lookup_off_the_128_byte_boundary(fl, kernel_policy, ty, policy):
    kernel_policy(policy)
    n = gs.aligned_column_blocks(1)
    T, esz = tbits(ty), tbits(ty) // 8
    N = 1 << T
    oracle = load_oracle()
    c = column_case(ty, n)                                                  # the key column: blocks on every 16-byte residue
    seed = seeds_from(83000 + 1000 * T + (policy != 0))
    # the value column: the key column's widths backwards, gaps of its own, references of its own
    widths, pad16, _ = gs.aligned_column_spec(ty, n)
    vw, voff, vcol, vblocks, _ = gs.mixed_column_host(ty, widths[::-1].copy(), 83100 + T, np.roll(pad16, 3))
    vrefs = gs.values(ty, n, 83200 + T)
    vvals = decode(oracle, ty, vblocks, vrefs)
    wk, wv = T // 2 + 1, 5
    pkk, pkv = gs.uniform_packed(ty, wk, n), gs.uniform_packed(ty, wv, n)
    keysu = oracle.batch("unfor_pack", ty, wk, pkk, aux=c["refs"], n_blocks=n)
    valsu = oracle.batch("unfor_pack", ty, wv, pkv, aux=vrefs, n_blocks=n)
    keep, words = column_masks(n, 83300 + n)
    narrow = int(np.argmin(np.where(c["widths"] >= 2, c["widths"], 99)))               # the narrowest block: a small window holds its keys
    lo = (int(c["refs"][narrow]) - 3) % N
    windows = [(lo, 40)] + ([((lo - 1000) % N, 8193)] if T > 8 else [])
    sentinel = np.full(256 * 4, SENTINEL, dtype=np.uint64).view(np.int64)
    for base in gs.ALIGNED_COLUMN_BASES:
        k = base // 16
        d_kcol, d_pkk = placed(c["col"], ty, base, gs.column_seed(ty, n, base)), placed(pkk, ty, base, gs.packed_seed(ty, wk, base))
        d_vcol, d_pkv = placed(vcol, ty, 96 - base, seed()), placed(pkv, ty, 96 - base, seed())
        d_kw, d_koff = placed(c["widths"], "uint8", 16 * (k + 1), seed()), placed(c["off"], "int64", 16 * (8 - k), seed())
        d_vw, d_voff = placed(vw, "uint8", 16 * (k + 2), seed()), placed(voff, "int64", 16 * (7 - k), seed())
        d_krefs, d_vrefs = placed(c["refs"], ty, esz, seed()), placed(vrefs, ty, 3 * esz, seed())
        d_m = placed(words, "int32", 16, seed())
        for q, (wlo, slots) in enumerate(windows):
            table, pw = code_table(slots, 83400 + slots % 1000), present_words(slots, 83500 + q)
            d_tb = placed(table, "u8", 16 * (1 + (k + q) % 7), seed())
            d_pr = placed(pw.view(np.int32), "int32", 16 * (1 + (k + 3 * q) % 7), seed())
            for form, vals, keys, ins in (("mixed", vvals, c["unfor_pack"], (d_vcol, d_vw, d_voff, d_vrefs, d_kcol, d_kw, d_koff, d_krefs)),
                                          ("uniform", valsu, keysu, (d_pkv, d_vrefs, d_pkk, d_krefs))):
                for j, (mask, kept, present) in enumerate(((d_m, keep, d_pr), (None, None, None))):
                    what = (ty, policy, n, base, form, slots, "mask" if mask else "no mask")
                    d_res = placed(sentinel, "int64", 16 * (1 + (k + 2 * q + j) % 7), seed())
                    d_st = placed(STATS_PREFILL.view(np.int64), "int64", 16 * (1 + (k + q + 3 * j) % 7), seed())
                    for p in (d_res, d_st, d_tb, d_pr):
                        assert p.t.data_ptr() % 128 and p.t.data_ptr() % 16 == 0
                    flag = zero_flag(seed())
                    tail = (mask.t.data_ptr() if mask else None, n, wlo, slots, d_tb.t.data_ptr(), present.t.data_ptr() if present else None,
                            d_res.t.data_ptr(), d_st.t.data_ptr(), flag.t.data_ptr())
                    if form == "mixed":
                        cabi(fl, f"fl_{ty}_{FORMS[1]}", d_vw.t.data_ptr(), d_voff.t.data_ptr(), d_vcol.t.data_ptr(), d_vcol.nbytes, d_vrefs.t.data_ptr(), 1,
                             d_kw.t.data_ptr(), d_koff.t.data_ptr(), d_kcol.t.data_ptr(), d_kcol.nbytes, d_krefs.t.data_ptr(), 1, *tail)
                    else:
                        cabi(fl, f"fl_{ty}_{FORMS[0]}", wv, d_pkv.t.data_ptr(), d_vrefs.t.data_ptr(), 1, wk, d_pkk.t.data_ptr(), d_krefs.t.data_ptr(), 1, *tail)
                    flag_clear(flag, what)
                    flag.check_guards(what)
                    want = expected_fused(ty, vals, keys, kept, wlo, table, pw if present else None, STATS_PREFILL)
                    if form == "mixed" and q == 0 and kept is None:
                        assert want[1][0] > STATS_PREFILL[0], what          # the small window is hit
                    same(d_res, want[0], what)
                    same(d_st, want[1], what)
                    guards(what, d_res, d_st, d_m, d_tb, d_pr, *ins)
