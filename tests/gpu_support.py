"""What the GPU tests share: the `fl` and `kernel_policy` fixtures (a test module takes them by import), host <-> device copies, and
the expected-value side of the FoR mask consumers' tests -- the mixed-width column, the mask set, numpy's comparison mask and the
per-block aggregates.  torch is imported inside the functions that need it: collecting the suite and the numpy half of this module
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


def mixed_column_host(ty, widths, seed):
    """(widths as uint8, int64 byte offset of every block, packed column, per-block (w, packed) for the oracle)"""
    esz = tbits(ty) // 8
    widths = np.asarray(widths).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum(widths.astype(np.int64) * 128)]) // esz
    col = values(ty, int(off[-1]), seed)
    return widths, (off[:-1] * esz).astype(np.int64), col, [(int(w), col[off[b]:off[b + 1]]) for b, w in enumerate(widths)]


def mixed_column(ty, widths, seed):
    """(device widths, device offsets, packed column, per-block (w, packed) for the oracle)"""
    import torch
    widths, off, col, blocks = mixed_column_host(ty, widths, seed)
    return torch.from_numpy(widths).cuda(), torch.from_numpy(off).cuda(), col, blocks


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
