"""GPU: unfor_aggregate_by_window / unfor_aggregate_by_window_widths with every device pointer off a 128-byte boundary, after the pattern
of tests/test_gpu_set_build_alignment.py (the padded mixed-width column whose blocks start on every 16-byte residue, the uniform
column, placed buffers with guard bytes): both packed columns at both bases, widths / offsets / references of either column, the mask
and err_flag at residues of their own, and the five buffers the call WRITES THROUGH -- counts, sums, mins, maxs and stats -- at 16-byte
offsets as well, in the LDS tier (40 groups) and above it (300 groups; 70001 for u32 / u64).  Every result is compared bit for bit with
numpy over the oracle's values on top of prefilled arrays and prefilled counters; after every call every byte outside every payload
must be what it was."""
import numpy as np
import pytest

import gpu_support as gs
from aggregate_by_window_data import STATS_PREFILL, expected_table, prefill_arrays
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TYS, placed
from oracle_lib import TYPES, load_oracle, tbits
from test_gpu_alignment import cabi, column_case, flag_clear, guards, same, seeds_from, zero_flag
from test_gpu_for_consumer_shapes import SHAPES, column_masks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("policy,bpw", SHAPES)
@pytest.mark.parametrize("ty", TYS)
def test_aggregate_by_window_off_the_128_byte_boundary(fl, kernel_policy, ty, policy, bpw):
    kernel_policy(policy)
    n = gs.aligned_column_blocks(bpw)
    T, esz = tbits(ty), tbits(ty) // 8
    N = 1 << T
    dt = TYPES[ty][0]
    c = column_case(ty, n)
    seed = seeds_from(99000 + 1000 * T + 10 * n)
    rng = np.random.default_rng(99400 + n)
    # the key column: the same packed bytes under references of its own, 60 keys apart around the small window (FoR: key = field +
    # reference); Python integers: they pass 2^63
    krefs = np.array([(N // 2 + 90 + int(x)) % N for x in rng.integers(0, 60, size=n)], dtype=np.uint64).astype(dt)
    with np.errstate(over="ignore"):
        keys_m = (c["unfor_pack"] - np.repeat(c["refs"], 1024) + np.repeat(krefs, 1024)).astype(dt)
    wu, wk = T // 2 + 1, 3
    pku, pkk = gs.uniform_packed(ty, wu, n), gs.uniform_packed(ty, wk, n)
    valsu = load_oracle().batch("unfor_pack", ty, wu, pku, aux=c["refs"], n_blocks=n)
    keys_u = load_oracle().batch("unfor_pack", ty, wk, pkk, aux=krefs, n_blocks=n)
    keep, words = column_masks(n, 99300 + n)
    lo = (N // 2 + 100) % N
    windows = [(lo, 40)] + ([((lo - 100) % N, 300)] if T > 8 else []) + ([((lo - 30000) % N, 70001)] if T > 16 else [])
    for base in gs.ALIGNED_COLUMN_BASES:
        k = base // 16
        d_col, d_key = placed(c["col"], ty, base, gs.column_seed(ty, n, base)), placed(c["col"], ty, 96 - base, seed())
        d_pku, d_pkk = placed(pku, ty, base, gs.packed_seed(ty, wu, base)), placed(pkk, ty, 96 - base, seed())
        d_w, d_off = placed(c["widths"], "uint8", 16 * (k + 1), seed()), placed(c["off"], "int64", 16 * (8 - k), seed())
        d_kw, d_koff = placed(c["widths"], "uint8", 16 * (7 - k), seed()), placed(c["off"], "int64", 16 * (k + 2), seed())
        d_refs, d_krefs = placed(c["refs"], ty, esz, seed()), placed(krefs, ty, 3 * esz, seed())
        d_m = placed(words, "int32", 16, seed())
        for q, (wlo, ng) in enumerate(windows):
            pre = prefill_arrays(ng, rng)
            for form, vals, keys, ins in (("mixed", c["unfor_pack"], keys_m, (d_col, d_key, d_w, d_off, d_kw, d_koff, d_refs, d_krefs)),
                                          ("uniform", valsu, keys_u, (d_pku, d_pkk, d_refs, d_krefs))):
                for j, (mask, kept) in enumerate(((d_m, keep), (None, None))):
                    what = (ty, policy, n, base, form, ng, "mask" if mask else "no mask")
                    d_arr = [placed(a.view(np.int64), "int64", 16 * (1 + (k + 2 * q + j + i) % 7), seed()) for i, a in enumerate(pre)]
                    d_st = placed(STATS_PREFILL.view(np.int64), "int64", 16 * (1 + (k + q + 3 * j) % 7), seed())
                    assert all(d.t.data_ptr() % 128 and d.t.data_ptr() % 16 == 0 for d in (*d_arr, d_st))
                    tail = (mask.t.data_ptr() if mask else None, n, wlo, ng, *(d.t.data_ptr() for d in d_arr), d_st.t.data_ptr())
                    if form == "mixed":
                        flag = zero_flag(seed())
                        cabi(fl, f"fl_{ty}_unfor_aggregate_by_window_widths", d_w.t.data_ptr(), d_off.t.data_ptr(), d_col.t.data_ptr(), d_col.nbytes,
                             d_refs.t.data_ptr(), 1, d_kw.t.data_ptr(), d_koff.t.data_ptr(), d_key.t.data_ptr(), d_key.nbytes, d_krefs.t.data_ptr(), 1,
                             *tail, flag.t.data_ptr())
                        flag_clear(flag, what)
                        flag.check_guards(what)
                    else:
                        cabi(fl, f"fl_{ty}_unfor_aggregate_by_window", wu, d_pku.t.data_ptr(), d_refs.t.data_ptr(), 1, wk, d_pkk.t.data_ptr(),
                             d_krefs.t.data_ptr(), 1, *tail)
                    want, want_stats = expected_table(ty, vals, keys, kept, wlo, ng, pre, STATS_PREFILL)
                    if kept is None:
                        assert want_stats[0] > STATS_PREFILL[0] and (q or want_stats[1] > STATS_PREFILL[1]), what
                    for d, w in zip(d_arr, want):
                        same(d, w, what)
                    same(d_st, want_stats, what)
                    guards(what, *d_arr, d_st, d_m, *ins)
