"""GPU: unfor_compare_in / unfor_compare_in_widths with every device pointer off a 128-byte boundary, after the pattern of
tests/test_gpu_alignment.py (its padded mixed-width column whose blocks start on every 16-byte residue, its uniform column, its placed
buffers with guard bytes): the packed column at both bases, widths / offsets / references / masks at residues of their own, and the
member set's bitmap -- set_words -- at a 16-byte offset as well, in the register tier (40 bits) and in the memory tier (2049 bits).
Every result is compared bit for bit with numpy over the oracle's values; after every call every byte outside every payload must be
what it was."""
import functools

import numpy as np
import pytest

import gpu_support as gs
from gpu_support import fl, kernel_policy  # noqa: F401 (fixtures)
from gpu_support import TYS, placed
from oracle_lib import load_oracle, tbits
from test_gpu_alignment import column_case, guards, same, seeds_from
from test_gpu_for_compare_in import Set, half, want_in
from test_gpu_for_compare_range import COMBINE
from test_gpu_for_consumer_shapes import SHAPES, column_masks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("policy,bpw", SHAPES)
@pytest.mark.parametrize("ty", TYS)
def test_compare_in_off_the_128_byte_boundary(fl, kernel_policy, ty, policy, bpw):
    kernel_policy(policy)
    n = gs.aligned_column_blocks(bpw)
    T, esz = tbits(ty), tbits(ty) // 8
    c = column_case(ty, n)
    seed = seeds_from(70000 + 1000 * T + 10 * n)
    wu = T // 2 + 1
    pku = gs.uniform_packed(ty, wu, n)
    valsu = load_oracle().batch("unfor_pack", ty, wu, pku, aux=c["refs"], n_blocks=n)
    bits, words = column_masks(n, 70300 + n)
    narrow = int(np.argmin(np.where(c["widths"] >= 2, c["widths"], 99)))               # the narrowest block: a small window holds its values
    rng = np.random.default_rng(70400 + n)
    lo = int(c["refs"][narrow]) - 3
    sets = [Set(ty, "40 bits", lo, 40, half(rng, 40, 3, 39), garbage=True)]
    if T > 8:
        sets.append(Set(ty, "2049 bits", lo - 1000, 2049, half(rng, 2049, 1003, 2048), garbage=True))
    for base in gs.ALIGNED_COLUMN_BASES:
        k = base // 16
        d_col, d_pku = placed(c["col"], ty, base, gs.column_seed(ty, n, base)), placed(pku, ty, base, gs.packed_seed(ty, wu, base))
        d_w, d_off = placed(c["widths"], "uint8", 16 * (k + 1), seed()), placed(c["off"], "int64", 16 * (8 - k), seed())
        d_refs = placed(c["refs"], ty, esz, seed())
        d_m = placed(words, "int32", 16, seed())
        for q, s in enumerate(sets):
            d_set = placed(s.words.view(np.int32), "int32", 16 * (1 + (k + 2 * q) % 7), seed())
            assert d_set.t.data_ptr() % 128 not in (0,) and d_set.t.data_ptr() % 16 == 0
            members = fl.MemberSet(ty, s.lo, s.bits, d_set.t)
            for form, vals, ins in (("mixed", c["unfor_pack"], (d_col, d_w, d_off, d_refs)), ("uniform", valsu, (d_pku, d_refs))):
                what = (ty, policy, n, base, form, s.name)
                call = functools.partial(fl.unfor_compare_in_widths, d_w.t, d_off.t, d_col.t, d_refs.t) if form == "mixed" else \
                    functools.partial(fl.FoR.unfor_compare_in, wu, d_pku.t, d_refs.t, n_blocks=n)
                if form == "mixed":
                    assert np.isin(vals, s.members).any(), what
                for j, cb in enumerate(COMBINE):
                    negate = (j + q) % 2 == 1
                    m = placed(n * 128, "int32", {1: (64, 80, 96), 5: (32, 48, 112)}[k][j], seed())
                    call(members, negate=negate, output=m.t, **(dict(mask=d_m.t, combine=cb) if cb != "new" else {}))
                    same(m, want_in(vals, s.members, negate, cb, words), what + (cb,))
                    guards(what + (cb,), m, d_m, d_set, *ins)
                m = placed(words, "int32", 16 * (8 - k), seed())
                call(members, mask=m.t, combine="or", output=m.t)
                same(m, want_in(vals, s.members, False, "or", words), what + ("or in place",))
                guards(what + ("or in place",), m, d_set, *ins)
