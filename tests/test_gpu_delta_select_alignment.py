"""GPU: undelta_select / undelta_select_widths with every device pointer at a merely-16-byte-aligned address inside a larger buffer, after
the pattern of tests/test_gpu_alignment.py (the padded mixed-width column whose blocks start on every 16-byte residue, the uniform column,
placed buffers with guard bytes): the packed column at both bases (residues 16 and 80), widths / offsets / bases / mask / out_offsets /
err_flag at residues of their own, and the output the call WRITES at further residues.  The column lengths are
gpu_support.ALIGNED_COLUMN_BLOCKS, each under the launch shape whose blocks per wavefront it was made for.  Every run is compared with
the oracle's untranspose(undelta_pack(..)) indexed by the mask's bits; after every call every byte outside every payload must be what
it was."""
import numpy as np
import pytest

import delta_compare_range_data as dd
import delta_select_data as ds
import gpu_support as gs
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import placed
from oracle_lib import load_oracle, tbits
from test_gpu_alignment import cabi, column_case, flag_clear, guards, same, seeds_from, zero_flag

pytestmark = pytest.mark.gpu

# blocks per wavefront -> the policy that forces it (1: the shipped shape; the others are served block by block)
SHAPES = {1: 0, 3: 2 + 256 * 6 + 65536 * 3, 4: 2 + 256 * 4 + 65536 * 4 + (1 << 24), 12: 2 + 256 * 4 + 65536 * 12 + (1 << 24)}
assert [gs.aligned_column_blocks(bpw) for bpw in SHAPES] == gs.ALIGNED_COLUMN_BLOCKS


@pytest.mark.parametrize("bpw", list(SHAPES))
@pytest.mark.parametrize("ty", gs.TYS)
def test_undelta_select_off_the_128_byte_boundary(fl, kernel_policy, ty, bpw):
    kernel_policy(SHAPES[bpw])
    n = gs.aligned_column_blocks(bpw)
    T = tbits(ty)
    c = column_case(ty, n)                                                  # blocks on every 16-byte residue; bases of its own
    bases = c["bases"]
    seed = seeds_from(87000 + 1000 * T + 10 * bpw)
    wu = T // 2 + 1
    pku = gs.uniform_packed(ty, wu, n)
    valsu = dd.decode_uniform(load_oracle(), ty, wu, pku, bases, n)
    masks = (dd.incoming_mask(n, 87300 + n, shift=bpw), np.packbits(np.random.default_rng(87400 + n).random(n * 1024) < 0.3, bitorder="little").view(np.int32))
    for base in gs.ALIGNED_COLUMN_BASES:
        k = base // 16
        d_col, d_pku = placed(c["col"], ty, base, gs.column_seed(ty, n, base)), placed(pku, ty, base, gs.packed_seed(ty, wu, base))
        d_w, d_off = placed(c["widths"], "uint8", 16 * (k + 1), seed()), placed(c["off"], "int64", 16 * (8 - k), seed())
        d_bases = placed(bases, ty, 16 * (k + 2), seed())
        assert d_col.t.data_ptr() % 128 == base == d_pku.t.data_ptr() % 128 and d_bases.t.data_ptr() % 128 == 16 * (k + 2)
        for form, vals, ins in (("mixed", c["undelta_pack_untranspose"], (d_col, d_w, d_off, d_bases)), ("uniform", valsu, (d_pku, d_bases))):
            for j, words in enumerate(masks):
                what = (ty, bpw, n, base, form, j)
                offsets, total = ds.offsets_of(words)
                assert total > 0
                d_m = placed(words, "int32", {1: 16, 5: 80}[k], seed())
                d_oo = placed(offsets, "int64", {1: 112, 5: 48}[k], seed())
                out = placed(total * (T // 8), ty, {1: (48, 96), 5: (16, 112)}[k][j], seed())
                assert out.t.data_ptr() % 128 != 0 and d_oo.t.data_ptr() % 128 != 0
                flag = zero_flag(seed())
                tail = (d_m.t.data_ptr(), d_oo.t.data_ptr(), out.t.data_ptr(), total, n, flag.t.data_ptr())
                if form == "mixed":
                    cabi(fl, f"fl_{ty}_{ds.FORMS[1]}", d_w.t.data_ptr(), d_off.t.data_ptr(), d_col.t.data_ptr(), d_col.nbytes, d_bases.t.data_ptr(), *tail)
                else:
                    cabi(fl, f"fl_{ty}_{ds.FORMS[0]}", wu, d_pku.t.data_ptr(), d_bases.t.data_ptr(), *tail)
                flag_clear(flag, what)
                flag.check_guards(what)
                same(out, ds.want_run(vals, words)[0], what)
                guards(what, out, d_m, d_oo, *ins)
