"""What the GPU tests share: the `fl` and `kernel_policy` fixtures (a test module takes them by import), host <-> device copies, and
the expected-value side of the FoR mask consumers' tests -- the mixed-width column, the mask set, numpy's comparison mask and the
per-block aggregates -- and buffers placed off the 128-byte boundary with the padded columns that go into them (placed,
aligned_column_host).  torch is imported inside the functions that need it: collecting the suite and the numpy half of this module
(tests/test_support_cpu.py pins it) need no GPU."""
import numpy as np
import pytest

from datagen import values
from oracle_lib import TYPES, tbits

TYS = ["u8", "u16", "u32", "u64"]
TDT = {"u8": "uint8", "u16": "uint16", "u32": "uint32", "u64": "uint64"}
SIGNED = {"u8": "uint8", "u16": "int16", "u32": "int32", "u64": "int64"}      # same-width dtypes torch compares / indexes / converts
POLICIES = [0, 1, 2, 2 + 256 * 4 + 65536 * 4 + (1 << 24), 2 + 256 * 6 + 65536 * 3]
GUARD = 96
CMP = {"==": np.equal, "!=": np.not_equal, "<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}
U64_MAX = np.uint64(2 ** 64 - 1)
IDENTITY = np.array([0, 0, 2 ** 64 - 1, 0], dtype=np.uint64)
SENTINEL = np.array(0xA5A5A5A5A5A5A5A5, dtype=np.uint64)


@pytest.fixture(scope="module")
def fl():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import fastlanes_amd
    fastlanes_amd.load()  # fails loudly if the HIP extension is missing
    return fastlanes_amd


@pytest.fixture
def kernel_policy(fl):
    """fl_internal_set_kernel_policy for one test, restored afterwards (0 automatic, 1 cell-column kernels, 2 wave-per-block)."""
    lib = fl.load()

    def set_policy(p):
        lib.fl_internal_set_kernel_policy(p)
        assert lib.fl_internal_get_kernel_policy() == p
    yield set_policy
    lib.fl_internal_set_kernel_policy(0)


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return torch.empty(0, dtype=getattr(torch, str(a.dtype)), device="cuda:0")
    return torch.from_numpy(a.view(np.uint8)).to("cuda:0").view(getattr(torch, str(a.dtype)))


def to_np(t, ty):
    """a contiguous CUDA tensor -> numpy in the type's own dtype (a view of the bytes: no copy is made to hide a stride)"""
    import torch
    assert t.is_contiguous(), (tuple(t.shape), t.stride())
    if t.numel() == 0:
        return np.zeros(0, dtype=TYPES[ty][0])
    return t.view(torch.uint8).cpu().numpy().view(TYPES[ty][0])


def u64_of(t):
    """a CUDA int64 tensor -> numpy uint64, same shape"""
    return t.contiguous().cpu().numpy().view(np.uint64)


def got_mask(t):
    return t.cpu().numpy().view(np.int32)


def mask_words(bits):
    """bool[n * 1024] -> the device mask: 32 int32 words per block, bit i of word i // 32, LSB first"""
    return to_dev(np.packbits(bits, bitorder="little").view(np.int32))


def want_mask(vals, op, k):
    """numpy's mask of unpacked values: 32 int32 words per 1024-value block, bit i of word i // 32, LSB first."""
    hit = CMP[op](vals, np.array(k, dtype=np.uint64).astype(vals.dtype))
    return np.packbits(hit, bitorder="little").view(np.int32)


def sentinel_of(ty):
    return SENTINEL.astype(TYPES[ty][0])


def sentinel_buffer(ty, n_elems):
    return to_dev(np.full(n_elems, sentinel_of(ty), dtype=TYPES[ty][0]))


def mixed_column_host(ty, widths, seed, pad16=None):
    """(widths as uint8, int64 byte offset of every block, packed column, per-block (w, packed) for the oracle).
    pad16: 16 * pad16[b] bytes of the column's own random stream lie in front of block b -- a column whose blocks start on any
    16-byte boundary, as fl_<ty>_unpack_widths allows -- and a fifth result follows: bool per byte of the column, True in the gaps."""
    esz = tbits(ty) // 8
    widths = np.asarray(widths).astype(np.uint8)
    if pad16 is None:
        off = np.concatenate([[0], np.cumsum(widths.astype(np.int64) * 128)]) // esz
        col = values(ty, int(off[-1]), seed)
        return widths, (off[:-1] * esz).astype(np.int64), col, [(int(w), col[off[b]:off[b + 1]]) for b, w in enumerate(widths)]
    pad = np.asarray(pad16).astype(np.int64) * 16
    assert pad.shape == widths.shape and (pad >= 0).all()
    size = widths.astype(np.int64) * 128
    off = np.cumsum(pad + size) - size                                          # the block's start: behind its own gap
    col = values(ty, int(off[-1] + size[-1]) // esz if widths.size else 0, seed)
    gaps = np.ones(col.nbytes, bool)
    for o, s in zip(off, size):
        gaps[o:o + s] = False
    blocks = [(int(w), col[o // esz:(o + s) // esz]) for w, o, s in zip(widths, off, size)]
    return widths, off.astype(np.int64), col, blocks, gaps


def mixed_column(ty, widths, seed, pad16=None):
    """(device widths, device offsets, packed column, per-block (w, packed) for the oracle[, the gaps' byte map])"""
    import torch
    widths, off, *rest = mixed_column_host(ty, widths, seed, pad16)
    return (torch.from_numpy(widths).cuda(), torch.from_numpy(off).cuda(), *rest)


# ---- buffers off the 128-byte boundary (tests/test_gpu_alignment.py; the conditions they rest on: tests/test_support_cpu.py) ----
PLACED_FRONT = 256                              # guard bytes in front of a placed payload, at least; at least as many follow it


def policy_bpw(policy):
    """blocks per wavefront of a kernel policy word of POLICIES / test_gpu_for_consumer_shapes.SHAPES: the cell-column kernels take
    one, the wave-per-block kernels the count in bits 16..23 (none given: at most 4)"""
    return 1 if policy == 1 else ((policy >> 16) & 0xFF) or 4


def aligned_column_blocks(bpw):
    """two full workgroups (4 wavefronts of bpw blocks), one more wavefront, and one block"""
    return 2 * 4 * bpw + bpw + 1


def aligned_column_spec(ty, n):
    """(widths, pad16, seed) of THE n-block column of `ty` whose blocks start on every 16-byte residue mod 128.
    Widths: 0 .. T in order where the column has room for them, otherwise an ascending sample of 0 .. T that keeps 0, T//2 - 1, T//2
    and T (both sides of the 2 * W >= T switch of the read route, and the ends); then seeded random ones.  Gaps: 48 bytes in front of
    each of the first nine blocks (the starts of the eight behind the width-0 block take all eight residues), then 0 .. 112 seeded
    random bytes."""
    T = tbits(ty)
    rs = np.random.default_rng(31000 + 64 * T + n)
    if n > T:
        widths = np.concatenate([np.arange(T + 1), rs.integers(0, T + 1, size=n - (T + 1))])
    else:
        widths = np.array(sorted({0, T // 2 - 1, T // 2, T} | {int(w) for w in np.round(np.linspace(0, T, n - 4))}))
        widths = np.concatenate([widths, rs.integers(0, T + 1, size=n - widths.size)])
    pad16 = np.concatenate([np.full(9, 3), rs.integers(0, 8, size=n - 9)])
    return widths.astype(np.int64), pad16.astype(np.int64), 31100 + 64 * T + n


def aligned_column_host(ty, n):
    widths, pad16, seed = aligned_column_spec(ty, n)
    return mixed_column_host(ty, widths, seed, pad16)


ALIGNED_COLUMN_BLOCKS = [aligned_column_blocks(bpw) for bpw in (1, 3, 4, 12)]    # every column length the alignment tests use
ALIGNED_COLUMN_BASES = (16, 80)                                                   # the residues their column base is placed at
UNIFORM_BLOCKS = 35                             # two full workgroups at 4 blocks per wavefront, and a tail of 3


def uniform_widths(ty):
    """both sides of the 2 * W >= T switch of the read route, and the ends"""
    T = tbits(ty)
    return [0, 1, T // 2 - 1, T // 2, T]


def uniform_packed(ty, w, n=UNIFORM_BLOCKS):
    return values(ty, n * 128 * w // (tbits(ty) // 8), 32000 + 64 * tbits(ty) + w)


def column_seed(ty, n, base):
    """the seed of the allocation that holds aligned_column_host(ty, n)'s column at the residue `base`"""
    return 34000 + 8 * (64 * tbits(ty) + n) + base // 16


def packed_seed(ty, w, residue):
    """the seed of the allocation (its guard bytes) that holds uniform_packed(ty, w) at `residue`"""
    return 33000 + 8 * (64 * tbits(ty) + w) + residue // 16


def slab_layout(sizes):
    """(start of every array, the slab's size), in bytes, for arrays sub-allocated from one slab: array a begins at the previous
    array's end rounded up to 16, plus 16 * (a % 8) bytes of filler -- neighbours lie 0 .. 112 bytes apart"""
    starts, pos = [], 0
    for a, size in enumerate(sizes):
        pos = -(-pos // 16) * 16 + 16 * (a % 8)
        starts.append(pos)
        pos += int(size)
    return starts, pos


def placed_image(payload, residue, seed, base=0):
    """(bytes, start): the image of one allocation at address `base` whose bytes [start, start + len(payload)) are `payload` (uint8)
    and lie at an address = residue mod 128, start >= PLACED_FRONT; seeded random bytes everywhere else, and PLACED_FRONT of them
    behind the payload.  The bytes in front of the payload are the END of one fixed stream per seed, so what precedes the payload
    does not depend on `base`: the CPU pins see the guard bytes the GPU run sees."""
    assert 0 <= residue < 128
    payload = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
    start = PLACED_FRONT + (residue - base - PLACED_FRONT) % 128
    noise = np.random.default_rng(seed).integers(0, 256, size=2 * (PLACED_FRONT + 128), dtype=np.uint8)
    half = PLACED_FRONT + 128
    return np.concatenate([noise[half - start:half], payload, noise[half:half + PLACED_FRONT]]), start


class Placed:
    """One raw CUDA allocation with a typed payload inside: `t` the payload's tensor, `check_guards()` that no byte outside it changed"""

    def __init__(self, raw, image, start, nbytes, ty):
        import torch
        self.raw, self.image, self.start, self.nbytes, self.ty = raw, image, start, nbytes, ty
        self.t = raw[start:start + nbytes].view(getattr(torch, TDT.get(ty, ty)))

    def np(self):
        """the payload as it is now, in its own dtype"""
        now = self.raw[self.start:self.start + self.nbytes].cpu().numpy()
        return now.view(TYPES[self.ty][0] if self.ty in TYPES else np.dtype(self.ty))

    def before(self):
        """the payload's bytes as they were written when the buffer was made (uint8)"""
        return self.image[self.start:self.start + self.nbytes].copy()

    def check_guards(self, what=None):
        now = self.raw.cpu().numpy()
        end = self.start + self.nbytes
        assert np.array_equal(now[:self.start], self.image[:self.start]), (what, "bytes in front of the buffer were written")
        assert np.array_equal(now[end:], self.image[end:]), (what, "bytes behind the buffer were written")


def placed(array_or_nbytes, ty, residue, seed):
    """A buffer at `residue` mod 128 inside a raw uint8 CUDA allocation of seeded random bytes (placed_image): the payload holds
    `array_or_nbytes`' bytes, or as many random ones.  `ty`: an element type of TYS, or a dtype name ("int32", "int64") for masks,
    slots and indices.  residue is a multiple of 16, or -- element-aligned buffers -- of the element size."""
    import torch
    esz = np.dtype(TDT.get(ty, ty)).itemsize
    assert residue % esz == 0
    if isinstance(array_or_nbytes, (int, np.integer)):
        payload = np.random.default_rng(seed + 1).integers(0, 256, size=int(array_or_nbytes), dtype=np.uint8)
    else:
        payload = np.ascontiguousarray(array_or_nbytes).view(np.uint8).reshape(-1)
    assert payload.size % esz == 0
    raw = torch.empty(payload.size + 2 * PLACED_FRONT + 128, dtype=torch.uint8, device="cuda:0")
    image, start = placed_image(payload, residue, seed, raw.data_ptr())
    assert image.size <= raw.numel() and start >= PLACED_FRONT and image.size - start - payload.size >= PLACED_FRONT
    raw = raw[:image.size]
    raw.copy_(torch.from_numpy(image))
    p = Placed(raw, image, start, payload.size, ty)
    assert (raw.data_ptr() + start) % 128 == residue
    assert payload.size == 0 or p.t.data_ptr() % 128 == residue, (p.t.data_ptr(), residue)
    return p


def mask_set(n, rng, full=True, with_none=False):
    """name -> bool[n * 1024]; with_none: plus "no mask" -> None, every row (the aggregate kernels take no mask at all)"""
    N = n * 1024
    out = {"zeros": np.zeros(N, bool), "ones": np.ones(N, bool)}
    for i in (0, 31, 32, 1022, 1023):
        m = np.zeros(N, bool)
        m[i::1024] = True
        out[f"bit {i}"] = m
    out["0xAAAAAAAA"] = np.arange(N) % 2 == 1
    for name, d in (("1/1024", 1 / 1024), ("1 %", 0.01), ("50 %", 0.5)):
        out[f"random {name}"] = rng.random(N) < d
    out["alternate"] = np.repeat(np.arange(n) % 2 == 1, 1024)
    last = np.zeros(N, bool)
    last[-1024:] = rng.random(1024) < 0.3
    out["last block only"] = last
    if not full:
        out = {k: out[k] for k in ("zeros", "ones", "bit 1023", "0xAAAAAAAA", "random 1 %", "random 50 %", "alternate", "last block only")}
    if with_none:
        out["no mask"] = None
    return out


def expected_blocks(vals, bits):
    """The reference: values (numpy over the oracle) and the mask's bits -> uint64[n, 4] = count, wrapping sum, min, max per block"""
    v = vals.reshape(-1, 1024).astype(np.uint64)
    b = np.ones(v.shape, bool) if bits is None else bits.reshape(-1, 1024)
    out = np.empty((v.shape[0], 4), dtype=np.uint64)
    out[:, 0] = b.sum(axis=1)
    out[:, 1] = np.where(b, v, np.uint64(0)).sum(axis=1, dtype=np.uint64)
    out[:, 2] = np.where(b, v, U64_MAX).min(axis=1)
    out[:, 3] = np.where(b, v, np.uint64(0)).max(axis=1)
    return out


def combine(slots):
    if slots.shape[0] == 0:
        return IDENTITY.copy()
    return np.array([slots[:, 0].sum(dtype=np.uint64), slots[:, 1].sum(dtype=np.uint64), slots[:, 2].min(), slots[:, 3].max()], dtype=np.uint64)


def sentinel_slots(n):
    """(the whole buffer, its first n slots as [n, 4]): sentinel-filled, GUARD slots behind"""
    import torch
    buf = to_dev(np.full((n + GUARD) * 4, SENTINEL, dtype=np.uint64).view(np.int64))
    assert buf.dtype == torch.int64
    return buf, buf[:n * 4].view(n, 4)


SLOTS = ("count", "sum", "min", "max")


def place(T, pos):
    """where an index-order position of a block sits: the row and lane a wavefront meets it in"""
    from extrema_data import row_lane
    r, l = row_lane(T, pos)
    return f"position {int(pos)} = row {r}, lane {l}"


def check_slots(buf, n, result, want, T, min_pos, max_pos, what, about=lambda b: ""):
    """The check of the one-element-decides tests (tests/test_gpu_extrema.py, tests/test_gpu_expr_extrema.py): all four slots of every
    block, the guard behind them and the combined result; the message names the first wrong block, the slot and where the block's
    extremes sit."""
    got = u64_of(buf)
    g = got[:n * 4].reshape(n, 4)
    if not np.array_equal(g, want):
        wrong = np.argwhere(g != want)
        b, s = (int(x) for x in wrong[0])
        raise AssertionError(f"{what}: {len(wrong)} slots differ, the first in block {b}{about(b)}: {SLOTS[s]} is {int(g[b, s])}, not {int(want[b, s])}; "
                             f"the block's minimum sits at {place(T, min_pos[b])}, its maximum at {place(T, max_pos[b])}")
    assert (got[n * 4:] == SENTINEL).all() and got.size == (n + GUARD) * 4, (what, "the guard was written")
    assert np.array_equal(u64_of(result), combine(want)), (what, "result", u64_of(result), combine(want))


class BackgroundLoad:
    """Keeps every CU busy on a SECOND stream while the kernels under test run on the current one: a queue of large decode
    launches (u32 W=20, 2 M blocks = 13 GB of traffic, ~2 ms each) refilled before every call under test."""

    def __init__(self, fl):
        import torch
        self.torch, self.fl = torch, fl
        self.stream = torch.cuda.Stream()
        n = 2_000_000
        self.pk = torch.empty(n * 640, dtype=torch.uint32, device="cuda:0")
        rc = fl.load().fl_fill_random(self.pk.data_ptr(), self.pk.numel() * 4, 3, None)
        assert rc == 0, (rc, fl.load().fl_last_hip_error())
        self.out = torch.empty(n * 1024, dtype=torch.uint32, device="cuda:0")
        torch.cuda.synchronize()

    def refill(self, launches=3):
        with self.torch.cuda.stream(self.stream):
            for _ in range(launches):
                self.fl.BitPacking.unpack(20, self.pk, output=self.out)

    def drain(self):
        self.stream.synchronize()
