"""What the unfor_aggregate_by tests share (tests/test_aggregate_by_cpu.py, tests/test_gpu_aggregate_by.py): the numpy reference of a
grouped aggregate -- np.add.at / np.minimum.at / np.maximum.at on uint64, 256 slots -- and u8 key columns of named distributions,
packed with the oracle's for_pack and decoded again with its unfor_pack (the decode is what the expected values come from).  numpy
only: no GPU is needed to import or use this module."""
import numpy as np

from gpu_support import IDENTITY

GROUPS = 256
KEY_KINDS = ("uniform", "four", "two", "clustered", "wrapping", "permutation", "constant")
KEY_WIDTH = {"uniform": 8, "four": 2, "two": 1, "clustered": 0, "wrapping": 3, "permutation": 8, "constant": 8}


def expected_groups(vals, keys, bits, without=()):
    """The reference: values (any unsigned dtype, zero-extended), their u8 keys and the mask's bits (None: every row) ->
    uint64[256, 4] = count, wrapping sum, min, max per key; a key that does not occur keeps the identity.  `without`: blocks that
    contribute nothing (skipped by the device checks)."""
    v = np.asarray(vals).reshape(-1).astype(np.uint64)
    k = np.asarray(keys).reshape(-1).astype(np.intp)
    assert v.size == k.size and v.size % 1024 == 0
    keep = np.ones(v.size, bool) if bits is None else np.asarray(bits).reshape(-1).copy()
    for b in without:
        keep[b * 1024:(b + 1) * 1024] = False
    v, k = v[keep], k[keep]
    out = np.tile(IDENTITY, (GROUPS, 1))
    count, total, lo, hi = (np.ascontiguousarray(out[:, j]) for j in range(4))
    np.add.at(count, k, np.uint64(1))
    np.add.at(total, k, v)                          # uint64: wraps mod 2^64
    np.minimum.at(lo, k, v)
    np.maximum.at(hi, k, v)
    return np.stack([count, total, lo, hi], axis=1)


def key_blocks(oracle, kind, n, rng):
    """n blocks of one key distribution: [(width, reference, packed uint8[128 * width])]
    uniform      every byte value, width 8                      four       only 0..3, width 2
    two          reference and reference + 1, width 1            clustered  width 0, the references cycle through 0, 7, 255
    wrapping     reference 250 at width 3: 250..255, 0, 1        constant   key 77 in every row, width 8
    permutation  every key exactly 4 times per block, width 8, a random (wrapping) reference"""
    w = KEY_WIDTH[kind]
    out = []
    for b in range(n):
        ref = {"uniform": 0, "four": 0, "clustered": (0, 7, 255)[b % 3], "wrapping": 250, "constant": 0}.get(kind)
        if ref is None:
            ref = int(rng.integers(0, 256))
        if kind == "permutation":
            pk = oracle.for_pack("u8", 8, rng.permutation(np.repeat(np.arange(256), 4)).astype(np.uint8), ref)
        elif kind == "constant":
            pk = oracle.for_pack("u8", 8, np.full(1024, 77, dtype=np.uint8), ref)
        else:
            pk = rng.integers(0, 256, size=128 * w, dtype=np.uint8)
        out.append((w, ref, np.asarray(pk, dtype=np.uint8)))
    return out


def key_column(oracle, blocks):
    """[(width, reference, packed)] -> (widths uint8[n], byte offsets int64[n], the packed column uint8, references uint8[n], the
    oracle's decode of every block: keys uint8[n * 1024])"""
    n = len(blocks)
    widths = np.array([w for w, _, _ in blocks], dtype=np.uint8)
    refs = np.array([r for _, r, _ in blocks], dtype=np.uint8)
    offsets = (np.concatenate([[0], np.cumsum(widths.astype(np.int64) * 128)])[:-1]).astype(np.int64)
    col = np.concatenate([pk for _, _, pk in blocks]) if n else np.zeros(0, np.uint8)
    keys = np.concatenate([oracle.unfor_pack("u8", int(w), pk, int(r)) for w, r, pk in blocks]) if n else np.zeros(0, np.uint8)
    return widths, offsets, col.astype(np.uint8), refs, keys.astype(np.uint8)
