"""GPU: unfor_set_build / unfor_set_build_widths with every device pointer off a 128-byte boundary, after the pattern of
tests/test_gpu_compare_in_alignment.py (the padded mixed-width column whose blocks start on every 16-byte residue, the uniform column,
placed buffers with guard bytes): the packed column at both bases, widths / offsets / references / mask / err_flag at residues of
their own, and the two buffers the call WRITES THROUGH -- set_words and stats -- at 16-byte offsets as well, in the LDS tier (40 bits)
and above it (2049 bits for u16, 70001 bits = the memory tier for u32 / u64).  Every result is compared bit for bit with numpy over the
oracle's values on top of a prefilled bitmap and prefilled counters; after every call every byte outside every payload must be what it
was."""
import numpy as np
import pytest

import gpu_support as gs
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TYS, placed
from oracle_lib import load_oracle, tbits
from set_build_data import STATS_PREFILL, expected_build, prefill_words
from test_gpu_alignment import cabi, column_case, flag_clear, guards, same, seeds_from, zero_flag
from test_gpu_for_consumer_shapes import SHAPES, column_masks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("policy,bpw", SHAPES)
@pytest.mark.parametrize("ty", TYS)
def test_set_build_off_the_128_byte_boundary(fl, kernel_policy, ty, policy, bpw):
    kernel_policy(policy)
    n = gs.aligned_column_blocks(bpw)
    T, esz = tbits(ty), tbits(ty) // 8
    N = 1 << T
    c = column_case(ty, n)
    seed = seeds_from(80000 + 1000 * T + 10 * n)
    wu = T // 2 + 1
    pku = gs.uniform_packed(ty, wu, n)
    valsu = load_oracle().batch("unfor_pack", ty, wu, pku, aux=c["refs"], n_blocks=n)
    keep, words = column_masks(n, 80300 + n)
    narrow = int(np.argmin(np.where(c["widths"] >= 2, c["widths"], 99)))               # the narrowest block: a small window holds its values
    rng = np.random.default_rng(80400 + n)
    lo = (int(c["refs"][narrow]) - 3) % N
    windows = [(lo, 40)] + ([((lo - 1000) % N, 2049 if T == 16 else 70001)] if T > 8 else [])
    for base in gs.ALIGNED_COLUMN_BASES:
        k = base // 16
        d_col, d_pku = placed(c["col"], ty, base, gs.column_seed(ty, n, base)), placed(pku, ty, base, gs.packed_seed(ty, wu, base))
        d_w, d_off = placed(c["widths"], "uint8", 16 * (k + 1), seed()), placed(c["off"], "int64", 16 * (8 - k), seed())
        d_refs = placed(c["refs"], ty, esz, seed())
        d_m = placed(words, "int32", 16, seed())
        for q, (wlo, bits) in enumerate(windows):
            pre = prefill_words(bits, rng)
            for form, vals, ins in (("mixed", c["unfor_pack"], (d_col, d_w, d_off, d_refs)), ("uniform", valsu, (d_pku, d_refs))):
                for j, (mask, kept) in enumerate(((d_m, keep), (None, None))):
                    what = (ty, policy, n, base, form, bits, "mask" if mask else "no mask")
                    d_set = placed(pre.view(np.int32), "int32", 16 * (1 + (k + 2 * q + j) % 7), seed())
                    d_st = placed(STATS_PREFILL.view(np.int64), "int64", 16 * (1 + (k + q + 3 * j) % 7), seed())
                    assert d_set.t.data_ptr() % 128 and d_set.t.data_ptr() % 16 == 0 and d_st.t.data_ptr() % 128 and d_st.t.data_ptr() % 16 == 0
                    tail = (mask.t.data_ptr() if mask else None, n, wlo, bits, d_set.t.data_ptr(), d_st.t.data_ptr())
                    if form == "mixed":
                        flag = zero_flag(seed())
                        cabi(fl, f"fl_{ty}_unfor_set_build_widths", d_w.t.data_ptr(), d_off.t.data_ptr(), d_col.t.data_ptr(), d_col.nbytes,
                             d_refs.t.data_ptr(), 1, *tail, flag.t.data_ptr())
                        flag_clear(flag, what)
                        flag.check_guards(what)
                    else:
                        cabi(fl, f"fl_{ty}_unfor_set_build", wu, d_pku.t.data_ptr(), d_refs.t.data_ptr(), 1, *tail)
                    want_words, want_stats = expected_build(ty, vals, kept, wlo, bits, pre, STATS_PREFILL)
                    if form == "mixed" and q == 0 and kept is None:
                        assert want_stats[0] > STATS_PREFILL[0], what
                    same(d_set, want_words, what)
                    same(d_st, want_stats, what)
                    guards(what, d_set, d_st, d_m, *ins)
