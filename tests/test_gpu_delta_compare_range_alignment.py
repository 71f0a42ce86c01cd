"""GPU: undelta_compare_range / undelta_compare_range_widths with every pointer argument at a merely-16-byte-aligned address inside a
larger buffer, after the pattern of tests/test_gpu_alignment.py (the padded mixed-width column whose blocks start on every 16-byte
residue, the uniform column, placed buffers with guard bytes): the packed column at both bases, widths / offsets / bases / mask_in /
err_flag at residues of their own, and the mask the call WRITES at further residues -- out of place under the three combiners, and in
place.  Every mask is compared with numpy over the oracle's untranspose(undelta_pack(..)); after every call every byte outside every
payload must be what it was."""
import numpy as np
import pytest

import delta_compare_range_data as dd
import gpu_support as gs
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import placed
from oracle_lib import load_oracle, tbits
from test_gpu_alignment import cabi, column_case, flag_clear, guards, same, seeds_from, zero_flag
from test_gpu_for_consumer_shapes import column_masks

pytestmark = pytest.mark.gpu

RUN_OF_3 = 2 + 256 * 6 + 65536 * 3                                              # a wavefront takes three blocks, one after the other


@pytest.mark.parametrize("policy", [0, RUN_OF_3], ids=["one block per wavefront", "runs of 3"])
@pytest.mark.parametrize("ty", gs.TYS)
def test_undelta_compare_range_off_the_128_byte_boundary(fl, kernel_policy, ty, policy):
    kernel_policy(policy)
    n = gs.aligned_column_blocks(1)
    T = tbits(ty)
    N = 1 << T
    c = column_case(ty, n)                                                  # blocks on every 16-byte residue; bases of its own
    bases = c["bases"]
    seed = seeds_from(84000 + 1000 * T + (policy != 0))
    wu = T // 2 + 1
    pku = gs.uniform_packed(ty, wu, n)
    valsu = dd.decode_uniform(load_oracle(), ty, wu, pku, bases, n)
    _, words = column_masks(n, 84300 + n)
    b0 = int(bases[(n // 2) * (1024 // T)])
    lo, hi = (b0 - (N >> 3)) % N, (b0 + (N >> 2)) % N
    for base in gs.ALIGNED_COLUMN_BASES:
        k = base // 16
        d_col, d_pku = placed(c["col"], ty, base, gs.column_seed(ty, n, base)), placed(pku, ty, base, gs.packed_seed(ty, wu, base))
        d_w, d_off = placed(c["widths"], "uint8", 16 * (k + 1), seed()), placed(c["off"], "int64", 16 * (8 - k), seed())
        d_bases = placed(bases, ty, 16 * (k + 2), seed())
        d_m = placed(words, "int32", 16, seed())
        assert d_col.t.data_ptr() % 128 == base == d_pku.t.data_ptr() % 128 and d_bases.t.data_ptr() % 128 == 16 * (k + 2)
        for form, vals, ins in (("mixed", c["undelta_pack_untranspose"], (d_col, d_w, d_off, d_bases)), ("uniform", valsu, (d_pku, d_bases))):
            for j, cb in enumerate(dd.COMBINE + ["and in place"]):
                what = (ty, policy, n, base, form, cb)
                inplace = cb == "and in place"
                code = 1 if inplace else j
                m = placed(words, "int32", 16 * (8 - k), seed()) if inplace else placed(n * 128, "int32", {1: (64, 80, 96), 5: (32, 48, 112)}[k][j], seed())
                assert m.t.data_ptr() % 128 not in (0, 16)
                mask_in = m if inplace else d_m
                flag = zero_flag(seed())
                tail = (lo, hi, code, mask_in.t.data_ptr() if code else None, n, m.t.data_ptr())
                if form == "mixed":
                    cabi(fl, f"fl_{ty}_{dd.FORMS[1]}", d_w.t.data_ptr(), d_off.t.data_ptr(), d_col.t.data_ptr(), d_col.nbytes, d_bases.t.data_ptr(), *tail,
                         flag.t.data_ptr())
                else:
                    cabi(fl, f"fl_{ty}_{dd.FORMS[0]}", wu, d_pku.t.data_ptr(), d_bases.t.data_ptr(), *tail)
                flag_clear(flag, what)
                flag.check_guards(what)
                same(m, dd.want_mask(vals, lo, hi, "and" if inplace else cb, words), what)
                guards(what, m, d_m, *ins)
