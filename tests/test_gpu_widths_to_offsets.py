"""GPU: fl_widths_to_offsets against a host prefix sum at its chunk edges.  The scan runs in three launches over chunks of 4096
blocks, with a second-level loop beyond 256 chunks (2^20 blocks); the parity tests compare it with a host prefix sum only inside one
chunk, and larger columns use its offsets on both sides of the comparison."""
import numpy as np
import pytest

from gpu_support import fl  # noqa: F401 (fixture)
from gpu_support import TYS
from oracle_lib import tbits

pytestmark = pytest.mark.gpu

COUNTS = [1, 4095, 4096, 4097, 8191, 8192, 8193, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 21) + 5]


def offsets_of(fl, ty, widths):
    import torch
    off, total = fl.widths_to_offsets(ty, torch.from_numpy(widths).cuda())
    return off.cpu().numpy(), int(total.item())


@pytest.mark.parametrize("ty", TYS)
def test_offsets_equal_the_host_prefix_sum_at_the_chunk_edges(fl, ty):
    """Seeded widths in 0..T: offsets[b] = sum of 128 * W over the blocks before b, total = the sum over all of them."""
    T = tbits(ty)
    for n in COUNTS:
        widths = np.random.default_rng(6100 + T + n).integers(0, T + 1, size=n).astype(np.uint8)
        want = np.concatenate([[0], np.cumsum(widths.astype(np.int64) * 128)])
        off, total = offsets_of(fl, ty, widths)
        assert off.dtype == np.int64 and off.size == n
        assert total == want[-1], (ty, n, total, int(want[-1]))
        bad = np.flatnonzero(off != want[:-1])
        assert bad.size == 0, (ty, n, f"{bad.size} offsets differ, the first at block {int(bad[0])}")


@pytest.mark.parametrize("ty", TYS)
def test_all_widest_blocks_past_the_second_level(fl, ty):
    """2^20 + 1 blocks of width T: the largest sums the column size allows per block."""
    T = tbits(ty)
    n = (1 << 20) + 1
    off, total = offsets_of(fl, ty, np.full(n, T, dtype=np.uint8))
    assert total == n * 128 * T
    assert np.array_equal(off, np.arange(n, dtype=np.int64) * (128 * T))


@pytest.mark.parametrize("ty", TYS)
def test_one_width_beyond_the_type_raises_wherever_it_is(fl, ty):
    """A single width T + 1 -- at the last block, at the first block of a chunk, in a chunk beyond the 256th -- sets the error flag
    (FL_ERR_WIDTH), and the same column without it does not."""
    T = tbits(ty)
    n = (1 << 20) + 3 * 4096 + 17
    base = np.random.default_rng(6200 + T).integers(0, T + 1, size=n).astype(np.uint8)
    offsets_of(fl, ty, base)
    for at in (n - 1, 4096, 5 * 4096, 257 * 4096, 258 * 4096 + 1234):
        widths = base.copy()
        widths[at] = T + 1
        with pytest.raises(fl.FastLanesError) as ei:
            offsets_of(fl, ty, widths)
        assert ei.value.status == 1, (ty, at, ei.value.status)
    for m, at in ((1, 0), (4097, 4096), (8192, 8191)):
        widths = base[:m].copy()
        widths[at] = T + 1
        with pytest.raises(fl.FastLanesError) as ei:
            offsets_of(fl, ty, widths)
        assert ei.value.status == 1, (ty, m, at)
