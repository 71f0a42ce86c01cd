"""Host-side mirror of the reference's codec traits over the C ABI.

The reference (a Rust crate; no Rust toolchain in this image) exposes static
trait methods per element type:

    BitPacking::{pack::<W>, unpack::<W>, unpack_single::<W>, unchecked_pack,
                 unchecked_unpack, unchecked_unpack_single}   (bitpacking.rs:16-59)
    FoR::{for_pack::<W>, unfor_pack::<W>}                     (ffor.rs:4-18)
    Delta::{delta, undelta, undelta_pack::<W>}                (delta.rs:6-17)
    Transpose::{transpose, untranspose}                       (transpose.rs:4-7)

This module keeps those names and argument meanings.  The element type is taken
from the array dtype (u8/u16/u32/u64 by item size), the const generic W becomes
the runtime `width` argument (as in the reference's own `unchecked_*` methods),
and every method is batched over `n_blocks = len(input) / block_len` contiguous
1024-value blocks (n_blocks = 1 is exactly one trait call).

* torch CUDA tensors  -> device tier (asynchronous on the current HIP stream)
* numpy arrays        -> host tier   (staged through device memory, synchronous)

Errors follow the reference: width > T and index >= 1024 are panics there
(bitpacking.rs:93,126,152,197) and raise FastLanesError here.  There is no CPU
implementation behind any of these calls.
"""
import ctypes

import numpy as np

from . import _lib

_NP = {1: "u8", 2: "u16", 4: "u32", 8: "u64"}
_NP_DTYPE = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64}


class FastLanesError(RuntimeError):
    def __init__(self, status, where):
        lib = _lib.load()
        msg = lib.fl_status_string(status).decode()
        if status == 5:
            msg += f" (hipError_t {lib.fl_last_hip_error()})"
        super().__init__(f"{where}: {msg}")
        self.status = status


def packed_len(ty, width):
    """bitpacking.rs:77: elements per packed block = 1024 * W / T."""
    return 1024 * width // _lib.BITS[ty]


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _ty_of(x):
    if _is_torch(x):
        return _NP[x.element_size()]
    return _NP[np.asarray(x).dtype.itemsize]


def _check(rc, where):
    if rc != 0:
        raise FastLanesError(rc, where)


# FL_DEVERR_* bits of a device error flag -> the fl_status a synchronous call would have returned
_DEVERR = ((1, 1), (2, 2), (8, 6), (4, 4))     # width, index, bounds, align (most specific first)


def _check_flag(err, where):
    bits = int(err.item())
    for bit, status in _DEVERR:
        if bits & bit:
            raise FastLanesError(status, where)
    if bits:
        raise FastLanesError(5, where)


class _Flag:
    """The device error flag of one call: a zeroed int32 word on `device` when the caller asked for the check (none otherwise),
    `ptr` for the C argument (None: the kernel reports nothing), `raise_if_set` after the launch -- the one sync of a checked call."""

    def __init__(self, check, device):
        import torch
        self.err = torch.zeros(1, dtype=torch.int32, device=device) if check else None
        self.ptr = self.err.data_ptr() if check else None

    def raise_if_set(self, where):
        if self.err is not None:
            _check_flag(self.err, where)


def _scalar(ty, value):
    """A Python int reduced mod 2^T, as the element type's C scalar (signed ints are reinterpreted, never refused)."""
    return _lib.CTYPE[ty](int(value) & ((1 << _lib.BITS[ty]) - 1))


def _indices(index, like):
    """Column-global element indices for the device tier: a CUDA int64/uint64 tensor on `like`'s device (anything
    else is converted from the host).  A float tensor, or one of another device, would be reinterpreted / fault."""
    import torch
    if _is_torch(index):
        if index.dtype not in (torch.int64, torch.uint64):
            raise TypeError(f"indices must be an int64/uint64 tensor, got {index.dtype}")
        idx = _Arg(index.contiguous(), "u64")
        _same_tier(like, idx)
        return idx.x
    a = np.asarray(index)
    if a.dtype.kind not in "ui":
        raise TypeError(f"indices must be integers, got dtype {a.dtype}")
    return torch.as_tensor(a.astype(np.int64).reshape(-1), device=like.x.device)


class _Arg:
    """Uniform view of a numpy array or a torch CUDA tensor."""

    def __init__(self, x, ty=None):
        self.torch = _is_torch(x)
        if self.torch:
            if not x.is_cuda:
                raise TypeError("torch tensors must live on the GPU (use numpy arrays for the host tier)")
            if not x.is_contiguous():
                raise ValueError("tensor must be contiguous")
            self.x = x
            self.n = x.numel()
            self.ptr = x.data_ptr()
        else:
            a = np.asarray(x)
            if a.dtype.kind not in "ui":
                raise TypeError(f"expected an unsigned integer array, got dtype {a.dtype}")
            if ty is not None and a.dtype.itemsize * 8 != _lib.BITS[ty]:
                raise TypeError(f"expected a {ty} array, got dtype {a.dtype}")
            if not a.flags["C_CONTIGUOUS"]:
                raise ValueError("array must be C-contiguous (an output would otherwise be written to a copy)")
            a = a.view(_NP_DTYPE[_NP[a.dtype.itemsize]])   # signed ints are reinterpreted, never converted
            self.x = a
            self.n = a.size
            self.ptr = a.ctypes.data
        self.ty = ty or _ty_of(x)
        if self.torch and ty is not None and x.element_size() * 8 != _lib.BITS[ty]:
            raise TypeError(f"expected a {ty} tensor, got dtype {x.dtype}")


def _empty_like(arg, n, ty):
    if arg.torch:
        import torch
        return torch.empty(n, dtype=arg.x.dtype, device=arg.x.device)
    return np.empty(n, dtype=_NP_DTYPE[ty])


def _stream(device):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _launch(name, device, *args, stream=True):
    """THE call into the C ABI: fetch `name` (`name`_host on the host tier, device=None), append the current HIP stream of `device`
    (stream=False: an entry point that takes none), call, and turn a non-zero status into FastLanesError.  The library launches on
    the calling thread's CURRENT device, so a tensor of another device is entered first -- and the stream is read inside that
    context; the common case, the tensor's device already current, skips the context switch."""
    fn = getattr(_lib.load(), name if device is not None else name + "_host")
    if device is None:
        rc = fn(*args)
    else:
        import torch
        if device.index == torch.cuda.current_device():
            rc = fn(*args, _stream(device)) if stream else fn(*args)
        else:
            with torch.cuda.device(device):
                rc = fn(*args, _stream(device)) if stream else fn(*args)
    _check(rc, name)


def _single_call(name, src, index, *lead):
    """The device tier of the two point lookups: `lead`, then (indices, n_indices, out, err_flag, stream).  The flag is always read
    back: an index past the column is the reference's assert (bitpacking.rs:152)."""
    import torch
    idx = _indices(index, src)
    out = torch.empty(idx.numel(), dtype=src.x.dtype, device=src.x.device)
    flag = _Flag(True, src.x.device)
    _launch(name, src.x.device, *lead, idx.data_ptr(), idx.numel(), out.data_ptr(), flag.ptr)
    flag.raise_if_set(name)
    return out


def _same_tier(src, *others):
    """Every buffer of one call lives on the same tier (all numpy, or all CUDA tensors of ONE device):
    a host pointer handed to a device kernel -- or a tensor of another GPU -- would fault the process."""
    for o in others:
        if o is None:
            continue
        if o.torch != src.torch:
            raise TypeError("input, output and base/reference must all be numpy arrays (host tier) or all be "
                            "CUDA tensors (device tier)")
        if src.torch and o.x.device != src.x.device:
            raise ValueError(f"tensors live on different devices ({src.x.device} vs {o.x.device})")


def _out(src, output, ty, n_elems, what):
    """The caller's output buffer (checked: a short buffer would be overrun by the kernel, which sizes
    its stores from n_blocks) or a fresh one.  Mirrors the reference's length asserts
    (bitpacking.rs:78-80,111-113)."""
    if output is None:
        return _Arg(_empty_like(src, n_elems, ty), ty)
    out = _Arg(output, ty)
    if out.n != n_elems:
        raise ValueError(f"{what}: output holds {out.n} elements, expected {n_elems}")
    return out


def _consumer_out(src, output, dtype, n_elems, what):
    """Output tensor of a fused consumer (sums / mask): the caller's CUDA tensor of exactly n_elems elements of `dtype`'s width on
    the input's device, or a fresh one.  (Where a thin output stream lives relative to the packed input moves the rate by
    10-15 %: DESIGN.md 4, fastlanes_amd/placement.py.)"""
    import torch
    if output is None:
        return torch.empty(n_elems, dtype=dtype, device=src.x.device)
    if not (_is_torch(output) and output.is_cuda and output.is_contiguous()):
        raise TypeError(f"{what}: output must be a contiguous CUDA tensor")
    if output.device != src.x.device:
        raise ValueError(f"tensors live on different devices ({src.x.device} vs {output.device})")
    if output.element_size() != torch.empty(0, dtype=dtype).element_size() or output.numel() != n_elems:
        raise ValueError(f"{what}: output holds {output.numel()} x {output.element_size()}-byte elements, expected {n_elems} x "
                         f"{torch.empty(0, dtype=dtype).element_size()}")
    return output


def _run(method, ty, width, src, out, n_blocks, aux=None, aux_stride=None, scalar=None):
    """Dispatch to fl_<ty>_<method>[_host]."""
    dev = src.torch
    _same_tier(src, out, aux)
    args = []
    if width is not None:
        args.append(width)
    args.append(src.ptr)
    if method in ("for_pack", "unfor_pack"):
        if dev:
            args += [aux.ptr, aux_stride]
        else:
            args.append(scalar)
    elif aux is not None:
        args.append(aux.ptr)
    _launch(f"fl_{ty}_{method}", src.x.device if dev else None, *args, out.ptr, n_blocks)
    return out.x


def _blocks(n, per_block, method):
    if per_block == 0:
        return None
    if n % per_block:
        raise ValueError(f"{method} input: length {n} is not a multiple of {per_block}")
    return n // per_block


def _check_width(ty, width, method):
    """width > T is unreachable!() in the reference (bitpacking.rs:93,126,197): FL_ERR_WIDTH here, before anything is sized from it."""
    if width > _lib.BITS[ty]:
        raise FastLanesError(1, f"fl_{ty}_{method}")


def _numel(x):
    return x.numel() if _is_torch(x) else np.asarray(x).size


def _uniform_blocks(src, width, method, n_blocks, *fallbacks):
    """Block count of a uniform-width packed input: the width check, then the packed length divided by the packed block
    (bitpacking.rs:77).  Width 0 packs to nothing, so the empty input says nothing: the count is then `n_blocks` if given, else that
    of the first `fallbacks` entry (tensor or None, its elements per block) that is there, else 0."""
    _check_width(src.ty, width, method)
    n = _blocks(src.n, packed_len(src.ty, width), method)
    if n is None:
        n = n_blocks if n_blocks is not None else next((_numel(t) // per for t, per in fallbacks if t is not None), 0)
    return n


def _block_words(x, what, words, word_bytes, src=None, n=None):
    """A per-block integer tensor of `words` `word_bytes`-byte words per block (a selection mask: 32 x 4, block aggregates: 4 x 8), on
    `src`'s tier and device when given: the wrapped tensor and its block count, which must be `n` when given."""
    a = _Arg(x)
    if src is not None:
        _same_tier(src, a)
    if a.x.dtype.is_floating_point or a.x.element_size() != word_bytes:
        raise TypeError(f"{what} must be an int{8 * word_bytes} / uint{8 * word_bytes} tensor ({words} words per block), got {a.x.dtype}")
    if n is not None and a.n != words * n:
        raise ValueError(f"{what} holds {a.n} words, expected {words} per block = {words * n}")
    if a.n % words:
        raise ValueError(f"{what} holds {a.n} words, not a multiple of {words} (one block)")
    return a, a.n // words


class BitPacking:
    """bitpacking.rs:16-59"""

    @staticmethod
    def pack(width, input, output=None):
        """BitPacking::pack::<W> / unchecked_pack (bitpacking.rs:19,30,65-96)."""
        src = _Arg(input)
        ty = src.ty
        _check_width(ty, width, "pack")
        n = _blocks(src.n, 1024, "pack")
        out = _out(src, output, ty, n * packed_len(ty, width), "pack")     # bitpacking.rs:78
        return _run("pack", ty, width, src, out, n)

    unchecked_pack = pack

    @staticmethod
    def unpack(width, input, output=None, n_blocks=None):
        """BitPacking::unpack::<W> / unchecked_unpack (bitpacking.rs:33,44,98-129).
        n_blocks is only needed for width == 0 (the packed input is empty)."""
        src = _Arg(input)
        ty = src.ty
        n = _uniform_blocks(src, width, "unpack", n_blocks, (output, 1024))
        out = _out(src, output, ty, n * 1024, "unpack")                    # bitpacking.rs:112
        return _run("unpack", ty, width, src, out, n)

    unchecked_unpack = unpack

    @staticmethod
    def unpack_single(width, packed, index, n_blocks=None):
        """BitPacking::unpack_single::<W> / unchecked_unpack_single (bitpacking.rs:47,58,132-200).
        `index` is an int (host tier: returns an int) or, on the device tier, a CUDA int64/uint64
        tensor of column-global element indices (block*1024 + i): returns a tensor of values."""
        src = _Arg(packed)
        ty = src.ty
        _check_width(ty, width, "unpack_single")
        pl = packed_len(ty, width)
        nb = n_blocks if n_blocks is not None else (src.n // pl if pl else 1)
        if not src.torch:
            val = _lib.CTYPE[ty](0)
            _launch(f"fl_{ty}_unpack_single", None, width, src.ptr, nb, int(index), ctypes.byref(val))
            return val.value
        return _single_call(f"fl_{ty}_unpack_single", src, index, width, src.ptr, nb)

    unchecked_unpack_single = unpack_single

    # ---- extensions -------------------------------------------------------
    @staticmethod
    def unpack_block_sums(width, packed, n_blocks=None, output=None):
        """sums[b] = sum(BitPacking.unpack(width, block b)) as wrapping uint64, without
        materialising the values.  Device tier only; returns a CUDA int64 tensor (bit pattern
        of the uint64 sums) -- `output` (n_blocks 8-byte elements) if given."""
        import torch
        src = _Arg(packed)
        n = _uniform_blocks(src, width, "unpack_block_sums", n_blocks)
        out = _consumer_out(src, output, torch.int64, n, "unpack_block_sums")
        _launch(f"fl_{src.ty}_unpack_block_sums", src.x.device, width, src.ptr, n, out.data_ptr())
        return out

    CMP = {"==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5}

    @staticmethod
    def unpack_compare(width, packed, op, constant, n_blocks=None, output=None):
        """Selection mask straight from packed data: bit i of block b's 1024-bit mask =
        (BitPacking.unpack(width, block b)[i] <op> constant), op in '==','!=','<','<=','>','>='.
        Device tier only; returns a CUDA int32 tensor of 32 words per block (bit i of word i//32,
        LSB first) -- `output` (32 * n_blocks 4-byte elements) if given."""
        import torch
        src = _Arg(packed)
        n = _uniform_blocks(src, width, "unpack_compare", n_blocks)
        out = _consumer_out(src, output, torch.int32, n * 32, "unpack_compare")
        _launch(f"fl_{src.ty}_unpack_compare", src.x.device, width, src.ptr, BitPacking.CMP[op], _scalar(src.ty, constant), n,
                out.data_ptr())
        return out

    @staticmethod
    def block_min_max(values, output=None):
        """(mins, maxs) per 1024-value block of an unpacked column -- written into `output` = (mins, maxs), two CUDA tensors of
        n_blocks elements of the column's type, if given.  Device tier only."""
        src = _Arg(values)
        n = _blocks(src.n, 1024, "block_min_max")
        mins, maxs = output if output is not None else (None, None)
        mins = _consumer_out(src, mins, src.x.dtype, n, "block_min_max mins")
        maxs = _consumer_out(src, maxs, src.x.dtype, n, "block_min_max maxs")
        _launch(f"fl_{src.ty}_block_min_max", src.x.device, src.ptr, n, mins.data_ptr(), maxs.data_ptr())
        return mins, maxs


class FoR:
    """ffor.rs:4-18.  `reference` is a scalar, or (device tier) a per-block CUDA tensor."""

    @staticmethod
    def _ref(src, ty, reference, n):
        if not src.torch:
            return None, None, _scalar(ty, reference)
        import torch
        if _is_torch(reference):
            r = _Arg(reference.contiguous(), ty)
            _same_tier(src, r)
            if r.n not in (1, n):
                raise ValueError("references must hold 1 or n_blocks elements")
            return r, (0 if r.n == 1 else 1), None
        host = np.array([_scalar(ty, reference).value], dtype=_NP_DTYPE[ty])
        r = torch.from_numpy(host.view(np.uint8)).to(src.x.device).view(src.x.dtype)
        return _Arg(r, ty), 0, None

    @staticmethod
    def for_pack(width, input, reference, output=None):
        """FoR::for_pack::<W> (ffor.rs:5-9,24-36)."""
        src = _Arg(input)
        ty = src.ty
        _check_width(ty, width, "for_pack")
        n = _blocks(src.n, 1024, "for_pack")
        out = _out(src, output, ty, n * packed_len(ty, width), "for_pack")
        aux, stride, scalar = FoR._ref(src, ty, reference, n)
        return _run("for_pack", ty, width, src, out, n, aux=aux, aux_stride=stride, scalar=scalar)

    @staticmethod
    def unfor_pack(width, input, reference, output=None, n_blocks=None):
        """FoR::unfor_pack::<W> (ffor.rs:11-17,38-50)."""
        src = _Arg(input)
        ty = src.ty
        n = _uniform_blocks(src, width, "unfor_pack", n_blocks, (output, 1024))
        out = _out(src, output, ty, n * 1024, "unfor_pack")
        aux, stride, scalar = FoR._ref(src, ty, reference, n)
        return _run("unfor_pack", ty, width, src, out, n, aux=aux, aux_stride=stride, scalar=scalar)

    # ---- extension -----------------------------------------------------------
    @staticmethod
    def unfor_compare(width, packed, reference, op, constant, n_blocks=None, output=None):
        """Selection mask straight from a FoR-packed column: bit i of block b's 1024-bit mask =
        (FoR.unfor_pack(width, block b, reference)[i] <op> constant), op in '==','!=','<','<=','>','>=' (unsigned,
        wrapping references allowed).  A block whose reference and width decide the predicate is answered without reading
        its packed bytes.  A plain bit-packed column is filtered with reference 0.  Device tier only; returns a CUDA int32
        tensor of 32 words per block (bit i of word i//32, LSB first) -- `output` (32 * n_blocks 4-byte elements) if given.
        n_blocks is only needed for width == 0."""
        import torch
        src = _Arg(packed)
        ty = src.ty
        if not src.torch:
            raise TypeError("unfor_compare is device tier (pass CUDA tensors)")
        n = _uniform_blocks(src, width, "unfor_compare", n_blocks, (output, 32))
        out = _consumer_out(src, output, torch.int32, n * 32, "unfor_compare")
        aux, stride, _ = FoR._ref(src, ty, reference, n)
        _launch(f"fl_{ty}_unfor_compare", src.x.device, width, src.ptr, aux.ptr, stride, BitPacking.CMP[op], _scalar(ty, constant), n,
                out.data_ptr())
        return out

    @staticmethod
    def unfor_compare_range(width, packed, reference, lo, hi, mask=None, combine="new", n_blocks=None, output=None):
        """Interval predicate chained through a mask: with v = FoR.unfor_pack(width, block b, reference)[i] and all arithmetic mod 2^T,
        hit = ((v - lo) mod 2^T) <= ((hi - lo) mod 2^T) -- the cyclic interval [lo, hi]: lo <= hi is BETWEEN, lo > hi wraps (v >= lo
        OR v <= hi), hi == lo - 1 matches every value; predicate_interval gives the interval of a comparison, signed ones included.
        combine "new": the result is hit (`mask` is ignored); "and" / "or": `mask` & hit / `mask` | hit, `mask` a CUDA int32 tensor of
        32 words per block (the layout unfor_compare returns).  A block its reference and width decide, a block whose `mask` is all
        zero under "and", and one whose `mask` is all ones under "or" are answered without reading their packed bytes.  `output` may
        be `mask` itself (in place).  Device tier only; returns a CUDA int32 tensor of 32 words per block (`output` if given).
        n_blocks is only needed for width == 0 without a mask or an output."""
        import torch
        cb = _range_combine(combine, mask)
        if cb and _is_torch(mask) and _is_torch(packed) and 0 < width <= _lib.BITS[_ty_of(packed)] and \
                mask.numel() * packed_len(_ty_of(packed), width) != 32 * packed.numel():
            raise ValueError(f"mask holds {mask.numel()} words, expected 32 per block of {packed_len(_ty_of(packed), width)} packed elements")
        src = _Arg(packed)
        ty = src.ty
        if not src.torch:
            raise TypeError("unfor_compare_range is device tier (pass CUDA tensors)")
        n = _uniform_blocks(src, width, "unfor_compare_range", n_blocks, (mask if cb and _is_torch(mask) else None, 32), (output, 32))
        m = _select_mask(src, mask, n) if cb else None
        out = _consumer_out(src, output, torch.int32, n * 32, "unfor_compare_range")
        aux, stride, _ = FoR._ref(src, ty, reference, n)
        _launch(f"fl_{ty}_unfor_compare_range", src.x.device, width, src.ptr, aux.ptr, stride, _scalar(ty, lo), _scalar(ty, hi), cb,
                m.ptr if m is not None and n else None, n, out.data_ptr())
        return out

    @staticmethod
    def unfor_compare_in(width, packed, reference, members, negate=False, mask=None, combine="new", n_blocks=None, output=None):
        """Set membership chained through a mask (WHERE x IN (...)): with v = FoR.unfor_pack(width, block b, reference)[i],
        hit = (v is a member of `members`) != negate.  `members` is a member_set result for the column's element type, or anything
        member_set accepts (it is then built here, on every call: build it once for a set that is used again).  combine "new": the
        result is hit (`mask` is ignored); "and" / "or": `mask` & hit / `mask` | hit, `mask` a CUDA int32 tensor of 32 words per block
        (the layout unfor_compare returns).  A block whose values all lie outside the set's window, a width-0 block, a block whose
        `mask` is all zero under "and", and one whose `mask` is all ones under "or" are answered without reading their packed bytes.
        `output` may be `mask` itself (in place).  Device tier only; returns a CUDA int32 tensor of 32 words per block (`output` if
        given).  n_blocks is only needed for width == 0 without a mask or an output."""
        import torch
        cb = _range_combine(combine, mask)
        if cb and _is_torch(mask) and _is_torch(packed) and 0 < width <= _lib.BITS[_ty_of(packed)] and \
                mask.numel() * packed_len(_ty_of(packed), width) != 32 * packed.numel():
            raise ValueError(f"mask holds {mask.numel()} words, expected 32 per block of {packed_len(_ty_of(packed), width)} packed elements")
        src = _Arg(packed)
        ty = src.ty
        if not src.torch:
            raise TypeError("unfor_compare_in is device tier (pass CUDA tensors)")
        n = _uniform_blocks(src, width, "unfor_compare_in", n_blocks, (mask if cb and _is_torch(mask) else None, 32), (output, 32))
        m = _select_mask(src, mask, n) if cb else None
        out = _consumer_out(src, output, torch.int32, n * 32, "unfor_compare_in")
        aux, stride, _ = FoR._ref(src, ty, reference, n)
        _launch(f"fl_{ty}_unfor_compare_in", src.x.device, width, src.ptr, aux.ptr, stride, *_member_args(ty, members, src.x.device),
                int(bool(negate)), cb, m.ptr if m is not None and n else None, n, out.data_ptr())
        return out

    @staticmethod
    def unfor_set_build(width, packed, reference, lo, bits, mask=None, into=None, n_blocks=None):
        """The member set of a column's values, built on the device (the build side of the semi-join unfor_compare_in probes): every
        v = FoR.unfor_pack(width, block b, reference)[i] in a row `mask` keeps (a CUDA int32 tensor of 32 words per block, the layout
        unfor_compare returns; None: every row) sets bit j = (v - lo) mod 2^T of the set when j < bits, and is counted as outside
        the window otherwise.  Returns (MemberSet, stats): the set (ty, lo, bits, words on the column's device) is usable in
        unfor_compare_in* as it stands; stats is a CUDA int64[2] tensor holding uint64 bits: kept rows inside, kept rows outside.
        `into`: a device MemberSet of the same ty, lo and bits, updated IN PLACE and returned (the union; stats counts this call
        alone).  A block whose mask is empty, a block outside the window and a width-0 block are answered without reading their
        packed bytes.  Device tier only.  n_blocks is only needed for width == 0 without a mask."""
        import torch
        src = _Arg(packed)
        ty = src.ty
        if not src.torch:
            raise TypeError("unfor_set_build is device tier (pass CUDA tensors)")
        n = _uniform_blocks(src, width, "unfor_set_build", n_blocks, (mask if _is_torch(mask) else None, 32))
        m = _select_mask(src, mask, n) if mask is not None else None
        ms = _set_build_target(ty, lo, bits, into, src.x.device)
        stats = torch.zeros(2, dtype=torch.int64, device=src.x.device)
        aux, stride, _ = FoR._ref(src, ty, reference, n)
        _launch(f"fl_{ty}_unfor_set_build", src.x.device, width, src.ptr, aux.ptr, stride, m.ptr if m is not None and n else None, n,
                _scalar(ty, ms.lo), ms.bits, ms.words.data_ptr() if ms.bits else None, stats.data_ptr())
        return ms, stats

    @staticmethod
    def unfor_lookup(width, packed, reference, lo, table, present=None, missing=0, mask=None, hit=None, output=None, stats=None, n_blocks=None):
        """The probe side of a payload join (unfor_lookup_widths' uniform form): for every row `mask` keeps (None: every row) with the
        key k = FoR.unfor_pack(width, block b, reference)[i] and j = (k - lo) mod 2^T, table[j] when j < len(table) and bit j of
        `present` (a MemberSet with the window lo, len(table); None: every slot) is set, `missing` otherwise.  `table`: a CUDA tensor
        of the key's own type or of uint8.  Returns (column, hit, stats) as unfor_lookup_widths does: the column in full-width packed
        order (fl.full_width_column), the hits as a mask (`hit=mask`: in place), stats += (hits, kept rows that miss).  Device tier
        only.  n_blocks is only needed for width == 0 without a mask, a hit or an output."""
        src = _Arg(packed)
        ty = src.ty
        if not src.torch:
            raise TypeError("unfor_lookup is device tier (pass CUDA tensors)")
        n = _uniform_blocks(src, width, "unfor_lookup", n_blocks, (mask if _is_torch(mask) else None, 32), (hit if _is_torch(hit) else None, 32),
                            (output, 1024))
        suffix, args, result = _lookup_args(src, n, lo, table, present, missing, mask, hit, output, stats)
        aux, stride, _ = FoR._ref(src, ty, reference, n)
        _launch(f"fl_{ty}_unfor_lookup{suffix}", src.x.device, width, src.ptr, aux.ptr, stride, *args)
        return result

    @staticmethod
    def unfor_aggregate_by_window(width, packed, reference, key_width, key_packed, key_reference, lo, n_groups, mask=None,
                                  what=("count", "sum"), into=None, n_blocks=None):
        """GROUP BY a key column of the value column's own type inside a dense window of the key domain: every row `mask` keeps (a
        CUDA int32 tensor of 32 words per block, the layout unfor_compare returns; None: every row) with the key k =
        FoR.unfor_pack(key_width, key_packed, key_reference)[i] updates slot j = (k - lo) mod 2^T of the arrays `what` names
        ("count", "sum", "min", "max") with the value FoR.unfor_pack(width, packed, reference)[i] when j < n_groups, and is counted
        as outside the window otherwise -- without materialising either column.  Returns (GroupTable, stats): the table's arrays
        are CUDA int64[n_groups] tensors holding uint64 bits (None for what is not named), freshly initialised to the identities
        0 / 0 / 2^64 - 1 / 0; stats is a CUDA int64[2] tensor holding uint64 bits: kept rows inside, kept rows outside.  `into`: a
        GroupTable of the same ty, lo, n_groups and arrays, updated IN PLACE and returned (stats counts this call alone).
        packed=None is the COUNT-only form: the key column stands in both places and what must be ("count",); without "sum", "min"
        and "max" the value column is never read.  A block whose mask is empty and a key block outside the window read neither
        column; a width-0 key block reads no key byte.  Device tier only.  n_blocks is only needed when both widths are 0 and
        there is no mask."""
        import torch
        names = _window_what(what)
        if packed is None:
            if names != ("count",):
                raise ValueError('packed=None is the COUNT-only form: what must be ("count",)')
            width, packed, reference = key_width, key_packed, key_reference
        src, ksrc = _Arg(packed), _Arg(key_packed)
        ty = src.ty
        if ksrc.ty != ty:
            raise TypeError(f"the key column must have the value column's element type, got {ksrc.ty} and {ty}")
        if not src.torch:
            raise TypeError("unfor_aggregate_by_window is device tier (pass CUDA tensors)")
        _same_tier(src, ksrc)
        _check_width(ty, key_width, "unfor_aggregate_by_window")
        n = _uniform_blocks(src, width, "unfor_aggregate_by_window", n_blocks, (key_packed if key_width else None, packed_len(ty, key_width)),
                            (mask if _is_torch(mask) else None, 32))
        if _uniform_blocks(ksrc, key_width, "unfor_aggregate_by_window", n) != n:
            raise ValueError(f"the key column does not hold the value column's {n} blocks")
        m = _select_mask(src, mask, n) if mask is not None else None
        table = _group_table_target(ty, lo, n_groups, names, into, src.x.device)
        stats = torch.zeros(2, dtype=torch.int64, device=src.x.device)
        aux, stride, _ = FoR._ref(src, ty, reference, n)
        kaux, kstride, _ = FoR._ref(ksrc, ty, key_reference, n)
        _launch(f"fl_{ty}_unfor_aggregate_by_window", src.x.device, width, src.ptr, aux.ptr, stride, key_width, ksrc.ptr, kaux.ptr, kstride,
                m.ptr if m is not None and n else None, n, _scalar(ty, table.lo), table.n_groups, *table._pointers(), stats.data_ptr())
        return table, stats

    @staticmethod
    def unfor_aggregate_by_lookup(width, packed, reference, key_width, key_packed, key_reference, lo, table, present=None, mask=None,
                                  n_blocks=None, result=None, stats=None):
        """GROUP BY a dimension attribute, fused (unfor_aggregate_by_lookup_widths' uniform form): every row `mask` keeps (None: every
        row) with the key k = FoR.unfor_pack(key_width, key_packed, key_reference)[i] and j = (k - lo) mod 2^T updates group table[j]
        (`table`: a CUDA uint8 tensor) with the value FoR.unfor_pack(width, packed, reference)[i] when j < len(table) and bit j of
        `present` (a MemberSet with the window lo, len(table); None: every slot) is set, and is counted as a miss otherwise -- FoR.unfor_lookup
        with a uint8 table followed by FoR.unfor_aggregate_by under the hits, with no code column and no hit mask written.  Returns
        (result, stats): a CUDA int64[256, 4] tensor (`result` if given) of count, sum, min, max per group, every row written by every
        call, and a CUDA int64[2] tensor holding uint64 bits, += (hits, kept rows that miss) (`stats` if given).  Device tier only.
        n_blocks is only needed when both widths are 0 and there is no mask."""
        src, ksrc = _Arg(packed), _Arg(key_packed)
        ty = src.ty
        if ksrc.ty != ty:
            raise TypeError(f"the key column must have the value column's element type, got {ksrc.ty} and {ty}")
        if not src.torch:
            raise TypeError("unfor_aggregate_by_lookup is device tier (pass CUDA tensors)")
        _same_tier(src, ksrc)
        _check_width(ty, key_width, "unfor_aggregate_by_lookup")
        n = _uniform_blocks(src, width, "unfor_aggregate_by_lookup", n_blocks, (key_packed if key_width else None, packed_len(ty, key_width)),
                            (mask if _is_torch(mask) else None, 32))
        if _uniform_blocks(ksrc, key_width, "unfor_aggregate_by_lookup", n) != n:
            raise ValueError(f"the key column does not hold the value column's {n} blocks")
        args, out = _aggregate_by_lookup_args("unfor_aggregate_by_lookup", src, n, lo, table, present, mask, result, stats)
        aux, stride, _ = FoR._ref(src, ty, reference, n)
        kaux, kstride, _ = FoR._ref(ksrc, ty, key_reference, n)
        _launch(f"fl_{ty}_unfor_aggregate_by_lookup", src.x.device, width, src.ptr, aux.ptr, stride, key_width, ksrc.ptr, kaux.ptr, kstride,
                *args, None)
        return out

    @staticmethod
    def unfor_compare_columns(width_a, a, a_reference, op, width_b, b, b_reference, *, signed=False, mask=None, combine="new", n_blocks=None,
                              output=None):
        """A predicate between two columns, chained through a mask: with va = FoR.unfor_pack(width_a, a block, a_reference)[i] and vb
        the same of column `b` (the same element type and block count; the widths may differ), hit = va <op> vb, op in '==', '!=',
        '<', '<=', '>', '>=' -- unsigned, or with signed=True of the two's-complement values.  combine "new": the result is hit
        (`mask` is ignored); "and" / "or": `mask` & hit / `mask` | hit, `mask` a CUDA int32 tensor of 32 words per block (the layout
        unfor_compare returns).  A block pair its references and widths decide, a block whose `mask` is all zero under "and", and one
        whose `mask` is all ones under "or" are answered without reading either column; a column of width 0 is never read.  `output`
        may be `mask` itself (in place).  Device tier only; returns a CUDA int32 tensor of 32 words per block (`output` if given).
        n_blocks is only needed when both widths are 0 and there is neither a mask nor an output."""
        import torch
        cb = _range_combine(combine, mask)
        sa, sb = _Arg(a), _Arg(b)
        ty = sa.ty
        if not sa.torch:
            raise TypeError("unfor_compare_columns is device tier (pass CUDA tensors)")
        if sb.ty != ty:
            raise TypeError(f"both columns must have one element type, got {ty} and {sb.ty}")
        _same_tier(sa, sb)
        _check_width(ty, width_b, "unfor_compare_columns")
        n = _uniform_blocks(sa, width_a, "unfor_compare_columns", n_blocks, (b if width_b else None, packed_len(ty, width_b)),
                            (mask if cb and _is_torch(mask) else None, 32), (output, 32))
        if _uniform_blocks(sb, width_b, "unfor_compare_columns", n) != n:
            raise ValueError(f"column b does not hold column a's {n} blocks")
        m = _select_mask(sa, mask, n) if cb else None
        out = _consumer_out(sa, output, torch.int32, n * 32, "unfor_compare_columns")
        ra, stride_a, _ = FoR._ref(sa, ty, a_reference, n)
        rb, stride_b, _ = FoR._ref(sb, ty, b_reference, n)
        _launch(f"fl_{ty}_unfor_compare_columns", sa.x.device, width_a, sa.ptr, ra.ptr, stride_a, width_b, sb.ptr, rb.ptr, stride_b,
                BitPacking.CMP[op], int(bool(signed)), cb, m.ptr if m is not None and n else None, n, out.data_ptr())
        return out

    @staticmethod
    def unfor_select(width, packed, reference, mask, out_offsets=None, total=None, n_blocks=None, output=None, check=True):
        """Only the rows a selection mask keeps: the values FoR.unfor_pack(width, packed, reference) yields where `mask` (the layout
        unfor_compare returns: a CUDA int32 tensor of 32 words per block, bit i of word i//32, LSB first) has a 1, compacted, in
        column order.  A block whose mask is empty is never read.  A plain bit-packed column is selected with reference 0.  Device
        tier only.  `out_offsets` / `total` are mask_offsets(mask)'s results (computed here if not given); with `output=None` the
        total is read back once to size the result (one sync), otherwise `output` receives the values and only its first `total`
        elements are written.  `check=True` reads the device error flag back (one sync) and raises if a block's run did not fit
        `output` (such a block is skipped either way); `check=False` stays asynchronous.  n_blocks is only needed for width == 0."""
        src = _Arg(packed)
        ty = src.ty
        if not src.torch:
            raise TypeError("unfor_select is device tier (pass CUDA tensors)")
        n = _uniform_blocks(src, width, "unfor_select", n_blocks, (mask if _is_torch(mask) else None, 32))
        aux, stride, _ = FoR._ref(src, ty, reference, n)
        return _select_call(f"fl_{ty}_unfor_select", src, n, (width, src.ptr, aux.ptr, stride), mask, out_offsets, total, output, check)

    @staticmethod
    def unfor_aggregate(width, packed, reference, mask=None, n_blocks=None, block_aggs=None, check=True):
        """COUNT / SUM / MIN / MAX of the values FoR.unfor_pack(width, packed, reference) yields where `mask` (the layout unfor_compare
        returns: a CUDA int32 tensor of 32 words per block) has a 1 -- `mask=None`: of every value, and no mask is read -- without
        materialising them.  Returns (result, block_aggs): `block_aggs` a CUDA int64[n_blocks, 4] tensor of the blocks' own
        aggregates (`block_aggs` if given), `result` a CUDA int64[4] tensor of their combination; both hold uint64 bit patterns in
        the order count, sum (wrapping mod 2^64), min, max; nothing kept gives (0, 0, 2^64 - 1, 0).  A block whose mask is empty, or
        whose width is 0, is never read.  A plain bit-packed column is aggregated with reference 0.  Device tier only; no host round
        trip (`check` only matters for the mixed-width form).  n_blocks is only needed for width == 0 without a mask."""
        src = _Arg(packed)
        ty = src.ty
        if not src.torch:
            raise TypeError("unfor_aggregate is device tier (pass CUDA tensors)")
        n = _uniform_blocks(src, width, "unfor_aggregate", n_blocks, (mask if _is_torch(mask) else None, 32))
        aux, stride, _ = FoR._ref(src, ty, reference, n)
        return _aggregate_call(f"fl_{ty}_unfor_aggregate", src, n, (width, src.ptr, aux.ptr, stride), mask, block_aggs, check)

    @staticmethod
    def unfor_aggregate_by(width, packed, reference, key_width, key_packed, key_reference, mask=None, n_blocks=None, result=None, check=True):
        """GROUP BY a u8 key: COUNT / SUM / MIN / MAX of the values FoR.unfor_pack(width, packed, reference) yields, grouped by the u8
        keys FoR.unfor_pack(key_width, key_packed, key_reference) yields in the same rows, where `mask` (the layout unfor_compare
        returns: a CUDA int32 tensor of 32 words per block; None: everywhere, and no mask is read) has a 1 -- without materialising
        either column.  Returns a CUDA int64[256, 4] tensor (`result` if given, 1024 8-byte elements): row g holds, as uint64 bit
        patterns, count, sum (wrapping mod 2^64), min, max of the kept rows whose key is g; a key that does not occur gives
        (0, 0, 2^64 - 1, 0).  Every row is written by every call.  A block whose mask is empty is never read; a key width of 0 (a
        column clustered by key) reads no key byte.  Deterministic.  Device tier only; no host round trip (`check` only matters for
        the mixed-width form).  n_blocks is only needed when both widths are 0 and there is no mask."""
        src, ksrc = _Arg(packed), _Arg(key_packed, "u8")
        ty = src.ty
        if not src.torch:
            raise TypeError("unfor_aggregate_by is device tier (pass CUDA tensors)")
        _same_tier(src, ksrc)
        _check_width("u8", key_width, "unfor_aggregate_by")
        n = _uniform_blocks(src, width, "unfor_aggregate_by", n_blocks, (key_packed if key_width else None, packed_len("u8", key_width)),
                            (mask if _is_torch(mask) else None, 32))
        if _uniform_blocks(ksrc, key_width, "unfor_aggregate_by", n) != n:
            raise ValueError(f"the key column does not hold the value column's {n} blocks")
        aux, stride, _ = FoR._ref(src, ty, reference, n)
        kaux, kstride, _ = FoR._ref(ksrc, "u8", key_reference, n)
        return _aggregate_by_call(f"fl_{ty}_unfor_aggregate_by", src, n, (width, src.ptr, aux.ptr, stride, key_width, ksrc.ptr, kaux.ptr, kstride),
                                  mask, result, check)

    EXPR = {"*": 0, "+": 1, "-": 2}         # include/fastlanes_amd.h: fl_expr

    @staticmethod
    def unfor_aggregate_columns(width_a, a, a_reference, expr, width_b, b, b_reference, mask=None, n_blocks=None, block_aggs=None,
                                check=True):
        """COUNT / SUM / MIN / MAX of an expression between two columns: with va = FoR.unfor_pack(width_a, a, a_reference)[i] and vb
        the same of column `b` (the same element type and block count; the widths may differ), x = va `expr` vb, expr one of '*',
        '+', '-' (a - b), over the rows where `mask` (the layout unfor_compare returns: a CUDA int32 tensor of 32 words per block;
        None: every row, and no mask is read) has a 1 -- SELECT SUM(price * discount) WHERE <mask>, without materialising either
        column.  Both values are zero-extended to 64 bits BEFORE the operation: u8 / u16 / u32 products and sums are exact, u64
        wraps; a difference below zero is its two's-complement bit pattern, so the sum is right as int64 and min / max compare the
        patterns as unsigned numbers.  Returns (result, block_aggs) as FoR.unfor_aggregate does: a CUDA int64[4] tensor and a CUDA
        int64[n_blocks, 4] tensor (`block_aggs` if given) of count, sum (wrapping mod 2^64), min, max as uint64 bit patterns;
        nothing kept gives (0, 0, 2^64 - 1, 0).  A block whose mask is empty, or whose two widths are both 0, reads neither column;
        a column of width 0 is never read.  Device tier only; no host round trip.  n_blocks is only needed when both widths are 0
        and there is no mask."""
        ex = _expr_code(expr)
        sa, sb = _Arg(a), _Arg(b)
        ty = sa.ty
        if sb.ty != ty:
            raise TypeError(f"both columns must have one element type, got {ty} and {sb.ty}")
        _check_width(ty, width_b, "unfor_aggregate_columns")
        n = _uniform_blocks(sa, width_a, "unfor_aggregate_columns", n_blocks, (b if width_b else None, packed_len(ty, width_b)),
                            (mask if _is_torch(mask) else None, 32))
        if _uniform_blocks(sb, width_b, "unfor_aggregate_columns", n) != n:
            raise ValueError(f"column b does not hold column a's {n} blocks")
        if not sa.torch:
            raise TypeError("unfor_aggregate_columns is device tier (pass CUDA tensors)")
        _same_tier(sa, sb)
        ra, stride_a, _ = FoR._ref(sa, ty, a_reference, n)
        rb, stride_b, _ = FoR._ref(sb, ty, b_reference, n)
        return _aggregate_call(f"fl_{ty}_unfor_aggregate_columns", sa, n,
                               (ex, width_a, sa.ptr, ra.ptr, stride_a, width_b, sb.ptr, rb.ptr, stride_b), mask, block_aggs, check)

    @staticmethod
    def unfor_aggregate_by_columns(width_a, a, a_reference, expr, width_b, b, b_reference, key_width, key_packed, key_reference,
                                   mask=None, n_blocks=None, result=None, check=True):
        """GROUP BY a u8 key of an expression between two columns: with va = FoR.unfor_pack(width_a, a, a_reference)[i], vb the same
        of column `b` (the same element type and block count; the widths may differ) and x = va `expr` vb, expr one of '*', '+', '-'
        (a - b), COUNT / SUM / MIN / MAX of x grouped by the u8 keys FoR.unfor_pack(key_width, key_packed, key_reference) yields in
        the same rows, where `mask` (the layout unfor_compare returns: a CUDA int32 tensor of 32 words per block; None: everywhere,
        and no mask is read) has a 1 -- SELECT k, SUM(price * discount) WHERE <mask> GROUP BY k, without materialising any of the
        three columns.  The values are those of FoR.unfor_aggregate_columns (zero-extended to 64 bits BEFORE the operation: u8 / u16
        / u32 exact, u64 wraps, a negative difference is its two's-complement pattern, min / max compare the patterns unsigned), the
        result is that of FoR.unfor_aggregate_by: a CUDA int64[256, 4] tensor (`result` if given), row g = count, sum, min, max of
        the kept rows whose key is g, (0, 0, 2^64 - 1, 0) for a key that does not occur; every row is written by every call.  A
        block whose mask is empty is never read; a key width of 0 reads no key byte; a column of width 0 is never read.
        Deterministic.  Device tier only; no host round trip.  n_blocks is only needed when all three widths are 0 and there is no
        mask.  SUM(a * (c - b)) per group is c * SUM(a) - SUM(a * b): one more FoR.unfor_aggregate_by launch."""
        ex = _expr_code(expr)
        sa, sb, ksrc = _Arg(a), _Arg(b), _Arg(key_packed, "u8")
        ty = sa.ty
        if sb.ty != ty:
            raise TypeError(f"both value columns must have one element type, got {ty} and {sb.ty}")
        _check_width(ty, width_b, "unfor_aggregate_by_columns")
        _check_width("u8", key_width, "unfor_aggregate_by_columns")
        n = _uniform_blocks(sa, width_a, "unfor_aggregate_by_columns", n_blocks, (b if width_b else None, packed_len(ty, width_b)),
                            (key_packed if key_width else None, packed_len("u8", key_width)), (mask if _is_torch(mask) else None, 32))
        if _uniform_blocks(sb, width_b, "unfor_aggregate_by_columns", n) != n:
            raise ValueError(f"column b does not hold column a's {n} blocks")
        if _uniform_blocks(ksrc, key_width, "unfor_aggregate_by_columns", n) != n:
            raise ValueError(f"the key column does not hold the value columns' {n} blocks")
        if not sa.torch:
            raise TypeError("unfor_aggregate_by_columns is device tier (pass CUDA tensors)")
        _same_tier(sa, sb, ksrc)
        ra, stride_a, _ = FoR._ref(sa, ty, a_reference, n)
        rb, stride_b, _ = FoR._ref(sb, ty, b_reference, n)
        kaux, kstride, _ = FoR._ref(ksrc, "u8", key_reference, n)
        return _aggregate_by_call(f"fl_{ty}_unfor_aggregate_by_columns", sa, n,
                                  (ex, width_a, sa.ptr, ra.ptr, stride_a, width_b, sb.ptr, rb.ptr, stride_b, key_width, ksrc.ptr, kaux.ptr, kstride),
                                  mask, result, check)


class Delta:
    """delta.rs:6-17.  `base` holds LANES = 1024/T elements per block."""

    @staticmethod
    def _go(method, width, input, base, output, per_block, n_blocks=None):
        src = _Arg(input)
        ty = src.ty
        if width is not None:
            _check_width(ty, width, method)
        n = _blocks(src.n, per_block(ty), method)
        b = _Arg(base, ty)
        if n is None:
            n = n_blocks if n_blocks is not None else b.n // (1024 // _lib.BITS[ty])
        if b.n != n * (1024 // _lib.BITS[ty]):
            raise ValueError("base must hold LANES elements per block")
        out = _out(src, output, ty, n * 1024, method)
        return _run(method, ty, width, src, out, n, aux=b)

    @staticmethod
    def delta(input, base, output=None):
        """Delta::delta (delta.rs:7,24-33)."""
        return Delta._go("delta", None, input, base, output, lambda ty: 1024)

    @staticmethod
    def undelta(input, base, output=None):
        """Delta::undelta (delta.rs:9,36-45)."""
        return Delta._go("undelta", None, input, base, output, lambda ty: 1024)

    @staticmethod
    def undelta_pack(width, input, base, output=None):
        """Delta::undelta_pack::<W> (delta.rs:11-16,47-63); output is in transposed order."""
        return Delta._go("undelta_pack", width, input, base, output, lambda ty: packed_len(ty, width))


    # ---- extensions: the compositions delta.rs:88-100 performs, in one pass ----
    @staticmethod
    def undelta_pack_untranspose(width, input, base, output=None):
        """== Transpose.untranspose(Delta.undelta_pack(width, input, base)): decodes straight to
        the ORIGINAL element order.  Device tier only."""
        if not _is_torch(input):
            raise TypeError("undelta_pack_untranspose is a device-tier extension (pass CUDA tensors)")
        return Delta._go("undelta_pack_untranspose", width, input, base, output, lambda ty: packed_len(ty, width))

    @staticmethod
    def undelta_compare_range(width, packed, base, lo, hi, mask=None, combine="new", n_blocks=None, output=None):
        """Interval predicate straight from a Delta-packed column, chained through a mask: with v = the values
        Delta.undelta_pack_untranspose(width, packed, base) yields (ORIGINAL row order) and all arithmetic mod 2^T, hit = ((v - lo) mod 2^T)
        <= ((hi - lo) mod 2^T) -- the cyclic interval [lo, hi] of FoR.unfor_compare_range, whose masks, `combine` names and in-place rule
        (`output` may be `mask` itself) these are: the result heads or joins any chain of the FoR consumers.  `base` holds LANES = 1024/T
        elements per block.  No decoded column is written: a block whose bases and width decide the interval (on a sorted column nearly
        every block), a width-0 block, a block whose `mask` is all zero under "and" and one whose `mask` is all ones under "or" are
        answered without reading their packed bytes.  Device tier only; returns a CUDA int32 tensor of 32 words per block (`output` if
        given).  n_blocks is only needed for width == 0 (default: from `base`)."""
        import torch
        cb = _range_combine(combine, mask)
        src = _Arg(packed)
        ty = src.ty
        if not src.torch:
            raise TypeError("undelta_compare_range is device tier (pass CUDA tensors)")
        lanes = 1024 // _lib.BITS[ty]
        if n_blocks is None and width == 0:
            n_blocks = _numel(base) // lanes
        n = _uniform_blocks(src, width, "undelta_compare_range", n_blocks, (mask if cb and _is_torch(mask) else None, 32), (output, 32))
        b, _ = _block_bases(src, ty, base, n)
        m = _select_mask(src, mask, n) if cb else None
        out = _consumer_out(src, output, torch.int32, n * 32, "undelta_compare_range")
        _launch(f"fl_{ty}_undelta_compare_range", src.x.device, width, src.ptr, b.ptr, _scalar(ty, lo), _scalar(ty, hi), cb,
                m.ptr if m is not None and n else None, n, out.data_ptr())
        return out

    @staticmethod
    def undelta_aggregate(width, packed, base, mask=None, n_blocks=None, block_aggs=None, check=True):
        """COUNT / SUM / MIN / MAX straight from a Delta-packed column: of the values Delta.undelta_pack_untranspose(width, packed, base)
        yields (ORIGINAL row order) where `mask` (the layout every compare writes and undelta_compare_range returns: a CUDA int32 tensor of
        32 words per block, bit i = original row i) has a 1 -- `mask=None`: of every value, and no mask is read -- without materialising
        them.  Returns (result, block_aggs) exactly as FoR.unfor_aggregate does: uint64 bit patterns count, sum (wrapping mod 2^64), min,
        max; nothing kept gives (0, 0, 2^64 - 1, 0).  `base` holds LANES = 1024/T elements per block.  A block whose mask is empty, or
        whose width is 0 (each lane's rows repeat its base), reads no packed byte.  Device tier only; no host round trip (`check` only
        matters for the mixed-width form).  n_blocks is only needed for width == 0 (default: from `base`)."""
        src = _Arg(packed)
        ty = src.ty
        if not src.torch:
            raise TypeError("undelta_aggregate is device tier (pass CUDA tensors)")
        lanes = 1024 // _lib.BITS[ty]
        if n_blocks is None and width == 0:
            n_blocks = _numel(base) // lanes
        n = _uniform_blocks(src, width, "undelta_aggregate", n_blocks, (mask if _is_torch(mask) else None, 32))
        b, _ = _block_bases(src, ty, base, n)
        return _aggregate_call(f"fl_{ty}_undelta_aggregate", src, n, (width, src.ptr, b.ptr), mask, block_aggs, check)

    @staticmethod
    def undelta_select(width, packed, base, mask, out_offsets=None, total=None, n_blocks=None, output=None, check=True):
        """Only the rows a selection mask keeps of a Delta-packed column: the values Delta.undelta_pack_untranspose(width, packed, base)
        yields (ORIGINAL row order) where `mask` (the layout every compare writes and undelta_compare_range returns: a CUDA int32 tensor of
        32 words per block, bit i = original row i) has a 1, compacted, in row order -- without writing the full-width column.  `base`
        holds LANES = 1024/T elements per block.  A block whose mask is empty is never read; a block of width 0 (each lane's rows repeat
        its base) reads no packed byte.  `out_offsets` / `total` / `output` / `check` are FoR.unfor_select's: mask_offsets(mask)'s results
        (computed here if not given), with `output=None` the total is read back once to size the result (one sync), and `check=True`
        reads the device error flag back (one sync) and raises if a block's run did not fit `output` (such a block is skipped either
        way).  Device tier only.  n_blocks is only needed for width == 0 (default: from `base`)."""
        src = _Arg(packed)
        ty = src.ty
        if not src.torch:
            raise TypeError("undelta_select is device tier (pass CUDA tensors)")
        lanes = 1024 // _lib.BITS[ty]
        if n_blocks is None and width == 0:
            n_blocks = _numel(base) // lanes
        n = _uniform_blocks(src, width, "undelta_select", n_blocks, (mask if _is_torch(mask) else None, 32))
        b, _ = _block_bases(src, ty, base, n)
        return _select_call(f"fl_{ty}_undelta_select", src, n, (width, src.ptr, b.ptr), mask, out_offsets, total, output, check)

    @staticmethod
    def transpose_delta_pack(width, input, base, output=None):
        """== BitPacking.pack(width, Delta.delta(Transpose.transpose(input), base)): encodes straight
        from the ORIGINAL element order.  Device tier only."""
        if not _is_torch(input):
            raise TypeError("transpose_delta_pack is a device-tier extension (pass CUDA tensors)")
        src = _Arg(input)
        ty = src.ty
        _check_width(ty, width, "transpose_delta_pack")
        n = _blocks(src.n, 1024, "transpose_delta_pack")
        b = _Arg(base, ty)
        if b.n != n * (1024 // _lib.BITS[ty]):
            raise ValueError("base must hold LANES elements per block")
        out = _out(src, output, ty, n * packed_len(ty, width), "transpose_delta_pack")
        return _run("transpose_delta_pack", ty, width, src, out, n, aux=b)


class Transpose:
    """transpose.rs:4-7"""

    @staticmethod
    def _go(method, input, output):
        src = _Arg(input)
        ty = src.ty
        n = _blocks(src.n, 1024, method)
        out = _out(src, output, ty, n * 1024, method)
        return _run(method, ty, None, src, out, n)

    @staticmethod
    def transpose(input, output=None):
        """Transpose::transpose (transpose.rs:5,11-15)."""
        return Transpose._go("transpose", input, output)

    @staticmethod
    def untranspose(input, output=None):
        """Transpose::untranspose (transpose.rs:6,17-22)."""
        return Transpose._go("untranspose", input, output)


def _check_widths_host(ty, widths):
    """Host widths -> contiguous uint8, refusing anything above T BEFORE the cast (300 must not wrap to 44)."""
    w = np.asarray(widths)
    if w.dtype.kind not in "ui":
        raise TypeError("widths must be an integer array")
    if w.size and (int(w.min()) < 0 or int(w.max()) > _lib.BITS[ty]):
        raise FastLanesError(1, "widths")                       # bitpacking.rs:93 unreachable!()
    return np.ascontiguousarray(w, dtype=np.uint8).reshape(-1)


def widths_to_offsets(ty, widths):
    """Device tier: (offsets, total) for a CUDA uint8 tensor of per-block widths -- offsets[b] = byte
    offset of block b in a back-to-back packed column (exclusive prefix sum of 128*W, bitpacking.rs:77),
    total = a 1-element CUDA int64 tensor holding the column's packed size.  No host round trip."""
    import torch
    w = _Arg(widths, "u8")
    if not w.torch:
        raise TypeError("widths_to_offsets is device tier (pass a CUDA uint8 tensor; sharding.packed_offsets is the host form)")
    dev = w.x.device
    offsets = torch.empty(w.n, dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    flag = _Flag(True, dev)
    _launch("fl_widths_to_offsets", dev, _lib.BITS[ty], w.ptr, w.n, offsets.data_ptr(), total.data_ptr(), flag.ptr)
    flag.raise_if_set("fl_widths_to_offsets")                   # bitpacking.rs:93 unreachable!()
    return offsets, total


# the packed side comes first for the decoders, last for the encoders; FoR's references / Delta's bases sit between the two sides
_WIDTHS_DECODERS = ("unpack_widths", "unfor_pack_widths", "undelta_pack_widths", "undelta_pack_untranspose_widths")


_NO_REFERENCES = object()


def _widths_column(method, packed, widths, offsets, *others, references=_NO_REFERENCES):
    """What every entry point over a mixed-width column opens with: `widths` as u8 and `offsets` as u64 on `packed`'s tier and device
    (`others`: further buffers of the call, checked first), device tier only, one offset per block, and -- for FoR's forms -- the
    blocks' references.  Returns the block count and the leading C arguments (widths, offsets, packed, packed_bytes[, references,
    reference_stride])."""
    w = _Arg(widths, "u8")
    o = _Arg(offsets, "u64")
    _same_tier(packed, *others, w, o)
    if not packed.torch:
        raise TypeError(f"{method} is device tier: widths, offsets and data must be CUDA tensors")
    n = w.n
    if o.n != n:
        raise ValueError("offsets must hold one entry per block")
    refs = _block_references(packed, packed.ty, references, n)[1] if references is not _NO_REFERENCES else ()
    pbytes = packed.n * (_lib.BITS[packed.ty] // 8)     # the kernel skips (and flags) any block that does not lie inside these bytes
    return n, (w.ptr, o.ptr, packed.ptr, pbytes, *refs)


def _widths_call(method, ty, widths, offsets, packed, unpacked, check, aux=()):
    """`aux`: the C arguments between the two sides -- (references pointer, stride) for FoR, (bases pointer,) for Delta."""
    n, (w, o, pk, pbytes) = _widths_column(method, packed, widths, offsets, unpacked)
    if unpacked.n != n * 1024:
        raise ValueError(f"{method}: the unpacked column must hold 1024 elements per block")
    flag = _Flag(check, packed.x.device)
    # C ABI argument order is (widths, offsets, in, [aux], out, ..): packed, packed_bytes -> unpacked for the decoders, the reverse
    # for the encoders
    args = (pk, pbytes, *aux, unpacked.ptr) if method in _WIDTHS_DECODERS else (unpacked.ptr, *aux, pk, pbytes)
    _launch(f"fl_{ty}_{method}", packed.x.device, w, o, *args, n, flag.ptr)
    flag.raise_if_set(f"fl_{ty}_{method}")                      # bitpacking.rs:93,126 unreachable!(); :78-80,111-113


def _block_references(src, ty, references, n):
    """FoR references of a mixed-width column: a CUDA tensor with one scalar per block, or one scalar for all (stride 0)."""
    r = _Arg(references, ty)
    _same_tier(src, r)
    if r.n not in (1, n):
        raise ValueError("references must hold one scalar per block (or exactly one, broadcast)")
    return r, (r.ptr, 0 if r.n == 1 and n != 1 else 1)


def _block_bases(src, ty, base, n):
    b = _Arg(base, ty)
    _same_tier(src, b)
    if b.n != n * (1024 // _lib.BITS[ty]):
        raise ValueError("base must hold LANES elements per block")
    return b, (b.ptr,)


def unpack_widths(widths, offsets, packed, output=None, check=True):
    """The reference's caller loop `for b: T::unchecked_unpack(widths[b], &packed[offsets[b]..], ..)`
    (bitpacking.rs:109-129) as ONE launch with everything device-resident: `widths` (CUDA uint8, one per
    block), `offsets` (CUDA int64/uint64 byte offsets into `packed`), `packed` (CUDA tensor of the element
    type).  `check=True` reads the device error flag back (one sync) and raises on a width > T, an
    offset that is not a multiple of 16, or a block that does not lie inside `packed` (the kernel skips such blocks
    either way); `check=False` stays asynchronous."""
    src = _Arg(packed)
    ty = src.ty
    n = _Arg(widths, "u8").n
    out = _out(src, output, ty, n * 1024, "unpack_widths")
    _widths_call("unpack_widths", ty, widths, offsets, src, out, check)
    return out.x


def pack_widths(widths, offsets, input, output, check=True):
    """`for b: T::unchecked_pack(widths[b], &input[b*1024..], &mut output[offsets[b]..])`
    (bitpacking.rs:76-96), device-resident.  `output` is the packed column (the caller sizes it from
    widths_to_offsets' total); bytes no block covers are left untouched."""
    src = _Arg(input)
    ty = src.ty
    out = _Arg(output, ty)
    _widths_call("pack_widths", ty, widths, offsets, out, src, check)
    return out.x


def unfor_pack_widths(widths, offsets, packed, references, output=None, check=True):
    """`for b: FoR::unfor_pack::<widths[b]>(&packed[offsets[b]..], references[b], ..)` (ffor.rs:38-50) -- unpack_widths with
    FoR's body; `references` is a CUDA tensor of one scalar per block (or a single one, broadcast)."""
    src = _Arg(packed)
    ty = src.ty
    n = _Arg(widths, "u8").n
    r, aux = _block_references(src, ty, references, n)
    out = _out(src, output, ty, n * 1024, "unfor_pack_widths")
    _widths_call("unfor_pack_widths", ty, widths, offsets, src, out, check, aux)
    return out.x


def unfor_compare_widths(widths, offsets, packed, references, op, constant, output=None, check=True):
    """FoR.unfor_compare over a mixed-width column: bit i of block b's 1024-bit mask =
    (FoR::unfor_pack::<widths[b]>(&packed[offsets[b]..], references[b])[i] <op> constant) -- `references` a CUDA tensor of one
    scalar per block (or a single one, broadcast).  A plain bit-packed mixed-width column is filtered with ONE zero reference
    (reference_stride 0).  Returns a CUDA int32 tensor of 32 words per block (`output` if given).  The per-block device checks
    of unfor_pack_widths: a block that fails them is skipped (its 32 mask words are left as they were); `check=True` reads the
    device error flag back (one sync) and raises, `check=False` stays asynchronous."""
    import torch
    src = _Arg(packed)
    ty = src.ty
    n, lead = _widths_column("unfor_compare_widths", src, widths, offsets, references=references)
    if op not in BitPacking.CMP:
        raise ValueError(f"op must be one of {sorted(BitPacking.CMP)}")
    out = _consumer_out(src, output, torch.int32, n * 32, "unfor_compare_widths")
    flag = _Flag(check, src.x.device)
    _launch(f"fl_{ty}_unfor_compare_widths", src.x.device, *lead, BitPacking.CMP[op], _scalar(ty, constant), n, out.data_ptr(), flag.ptr)
    flag.raise_if_set(f"fl_{ty}_unfor_compare_widths")          # bitpacking.rs:93,126 unreachable!(); :111-113
    return out


def _select_mask(src, mask, n):
    """The selection mask of a select call: a CUDA tensor of 32 four-byte integer words per block, on the column's device."""
    return _block_words(mask, "mask", 32, 4, src, n)[0]


def _range_combine(combine, mask):
    """fl_mask_combine of a combine name; "and" / "or" need the mask so far."""
    if combine not in _lib.MASK_COMBINE:
        raise ValueError(f"combine must be one of {sorted(_lib.MASK_COMBINE)}")
    cb = _lib.MASK_COMBINE[combine]
    if cb and mask is None:
        raise ValueError(f'combine="{combine}" needs the mask so far')
    return cb


def predicate_interval(ty, op, constant, signed=False):
    """The cyclic interval (lo, hi) of bit patterns that satisfy `v <op> constant` for an element type ("u8" .. "u64") -- what
    unfor_compare_range takes -- or None when no value satisfies it (x < 0 unsigned, x > the largest value, ...).  op is one of
    '==', '!=', '<', '<=', '>', '>='.  signed=False compares unsigned (the constant is taken mod 2^T, as unfor_compare does);
    signed=True reads the element type as two's complement, the constant within [-2^(T-1), 2^(T-1) - 1]: the signed order runs from
    the pattern 2^(T-1) up through 2^T - 1, wraps to 0 and ends at 2^(T-1) - 1, so `x < k` is [2^(T-1), k - 1] -- a cyclic interval,
    and every comparison of a signed column is one.  Pure Python, no GPU.
    A predicate that no value satisfies has no interval: the caller skips the call and uses a zero mask under combine "new" / "and",
    the mask so far under "or".  The complement of [lo, hi] is [hi + 1, lo - 1] (mod 2^T) unless the interval is full (hi == lo - 1),
    whose complement is empty: NOT / AND-NOT are expressed through it."""
    T = _lib.BITS[ty]
    M = (1 << T) - 1
    if op not in BitPacking.CMP:
        raise ValueError(f"op must be one of {sorted(BitPacking.CMP)}")
    k = int(constant)
    if signed:
        if not -(1 << (T - 1)) <= k < (1 << (T - 1)):
            raise ValueError(f"constant {k} is not an i{T}")
        first, last = 1 << (T - 1), (1 << (T - 1)) - 1       # the patterns of the smallest and the largest value
    else:
        first, last = 0, M
    k &= M
    if op == "==":
        return k, k
    if op == "!=":
        return (k + 1) & M, (k - 1) & M
    if op == "<":
        return None if k == first else (first, (k - 1) & M)
    if op == "<=":
        return first, k
    if op == ">":
        return None if k == last else ((k + 1) & M, last)
    return k, last


def unfor_compare_range_widths(widths, offsets, packed, references, lo, hi, mask=None, combine="new", output=None, check=True):
    """FoR.unfor_compare_range over a mixed-width column: the cyclic interval [lo, hi] (mod 2^T; predicate_interval gives a
    comparison's) over the values unfor_pack_widths(widths, offsets, packed, references) yields, joined with the mask so far --
    combine "new": the hits themselves (`mask` is ignored), "and" / "or": `mask` & hits / `mask` | hits.  `mask` and the result are
    CUDA int32 tensors of 32 words per block (unfor_compare_widths' layout); `output` may be `mask` itself (in place).  A block its
    reference and width decide, a block whose `mask` is all zero under "and", and one whose `mask` is all ones under "or" are
    answered without reading their packed bytes -- so the later predicates of a chain read only the blocks the earlier ones left
    open.  The per-block device checks of unfor_compare_widths, with the same contract: a block that fails them is skipped (its 32
    mask words are left as they were); `check=True` reads the device error flag back (one sync) and raises, `check=False` stays
    asynchronous."""
    import torch
    cb = _range_combine(combine, mask)
    if cb and _is_torch(mask) and _is_torch(widths) and mask.numel() != 32 * widths.numel():
        raise ValueError(f"mask holds {mask.numel()} words, expected 32 per block = {32 * widths.numel()}")
    src = _Arg(packed)
    ty = src.ty
    n, lead = _widths_column("unfor_compare_range_widths", src, widths, offsets, references=references)
    m = _select_mask(src, mask, n) if cb else None
    out = _consumer_out(src, output, torch.int32, n * 32, "unfor_compare_range_widths")
    flag = _Flag(check, src.x.device)
    _launch(f"fl_{ty}_unfor_compare_range_widths", src.x.device, *lead, _scalar(ty, lo), _scalar(ty, hi), cb,
            m.ptr if m is not None and n else None, n, out.data_ptr(), flag.ptr)
    flag.raise_if_set(f"fl_{ty}_unfor_compare_range_widths")    # bitpacking.rs:93,126 unreachable!(); :111-113
    return out


class MemberSet:
    """A member set for unfor_compare_in (member_set builds it): the element type `ty`, and a window of the value domain plus a
    bitmap -- bit j of `words` (bit j % 32 of word j // 32), 0 <= j < `bits`, says whether the bit pattern (`lo` + j) mod 2^T is a
    member.  `words` is a numpy uint32 array, or a CUDA int32 tensor when the set was built for a device; on(device) is the bitmap on
    that device (uploaded once per device and kept)."""
    __slots__ = ("ty", "lo", "bits", "words", "_on")

    def __init__(self, ty, lo, bits, words):
        self.ty, self.lo, self.bits, self.words, self._on = ty, lo, bits, words, {}

    def __iter__(self):
        return iter((self.ty, self.lo, self.bits, self.words))

    def __repr__(self):
        return f"MemberSet({self.ty}, lo={self.lo}, bits={self.bits})"

    def on(self, device):
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if _is_torch(self.words):
            if self.words.device != device:
                raise ValueError(f"tensors live on different devices ({device} vs {self.words.device})")
            return self.words
        if device not in self._on:
            self._on[device] = torch.from_numpy(self.words.view(np.int32)).to(device)
        return self._on[device]


def _member_patterns(ty, members, signed):
    """The distinct bit patterns of `members`, ascending, as numpy uint64."""
    T = _lib.BITS[ty]
    M = (1 << T) - 1
    if _is_torch(members):
        if members.dtype.is_floating_point:
            raise TypeError(f"members must be integers, got {members.dtype}")
        members = members.detach().cpu().contiguous().numpy()
    if isinstance(members, np.ndarray):
        if members.dtype.kind not in "ui":
            raise TypeError(f"members must be integers, got dtype {members.dtype}")
        a = members.reshape(-1)
        lo, hi = (-(1 << (T - 1)), (1 << (T - 1)) - 1) if signed else (0, M)
        if a.size and (int(a.min()) < lo or int(a.max()) > hi):
            raise ValueError(f"members must lie in [{lo}, {hi}] ({'i' if signed else 'u'}{T})")
        if a.dtype.kind == "i":
            a = a.astype(np.int64).view(np.uint64)                         # two's complement, sign-extended to 64 bits
        return np.unique(a.astype(np.uint64) & np.uint64(M))
    vals = [int(v) for v in members]
    lo, hi = (-(1 << (T - 1)), (1 << (T - 1)) - 1) if signed else (0, M)
    if any(v < lo or v > hi for v in vals):
        raise ValueError(f"members must lie in [{lo}, {hi}] ({'i' if signed else 'u'}{T})")
    return np.unique(np.array([v & M for v in vals], dtype=np.uint64))


def member_set(ty, members, signed=False, max_bits=1 << 27, device=None):
    """The member set of `members` for unfor_compare_in over a column of element type `ty` ("u8" .. "u64"): a MemberSet (ty, lo,
    bits, words).  `members`: an iterable, a numpy array or a torch tensor of integers -- values of the element type, or with
    signed=True two's-complement values within [-2^(T-1), 2^(T-1) - 1]; duplicates are fine.  The window is the TIGHTEST cyclic one:
    the distinct bit patterns are sorted, the cycle 0 .. 2^T - 1 .. 0 is cut at its largest gap (on ties: the cut that gives the
    smallest `lo`), so {-1, 0, 1} of a signed u32 column is 3 bits at lo = 2^32 - 1, not 2^32 bits.  The empty set has bits = 0 and
    no words.  Bits past `bits` in the last word are clear.  A window of more than `max_bits` bits (the default is a 16-MiB bitmap),
    or of more than 2^32, raises ValueError: such a set is a join, not a filter.  device: None keeps `words` on the host (a call
    uploads it to the column's device and keeps it there); a CUDA device puts it there now."""
    if ty not in _lib.BITS:
        raise ValueError(f"ty must be one of {list(_lib.TYPES)}")
    T = _lib.BITS[ty]
    N, M = 1 << T, (1 << T) - 1
    p = _member_patterns(ty, members, signed)
    k = p.size
    if k == 0:
        lo, bits = 0, 0
    elif k == 1:
        lo, bits = int(p[0]), 1
    else:
        gaps = np.concatenate([np.diff(p), (p[:1] - p[-1:]) & np.uint64(M)])   # gaps[i]: from p[i] to its successor on the cycle
        starts = np.roll(p, -1)[gaps == gaps.max()]                             # the window begins behind a largest gap
        lo, bits = int(starts.min()), N - int(gaps.max()) + 1
    if bits > max_bits or bits > min(N, 1 << 32):
        raise ValueError(f"member_set: the tightest window holds {bits} bits, more than max_bits = {min(max_bits, N, 1 << 32)}")
    words = np.zeros((bits + 31) // 32, dtype=np.uint32)
    if k:
        j = (p - np.uint64(lo)) & np.uint64(M)
        np.bitwise_or.at(words, (j >> np.uint64(5)).astype(np.int64), np.uint32(1) << (j & np.uint64(31)).astype(np.uint32))
    ms = MemberSet(ty, lo, bits, words)
    if device is not None:
        ms.words = ms.on(device)
    return ms


def _member_args(ty, members, device):
    """(set_lo, set_bits, set_words) of a call on `device`: `members` a MemberSet of the column's type, or anything member_set takes"""
    ms = members if isinstance(members, MemberSet) else member_set(ty, members)
    if ms.ty != ty:
        raise TypeError(f"the member set is of {ms.ty}, the column of {ty}")
    return _scalar(ty, ms.lo), ms.bits, ms.on(device).data_ptr() if ms.bits else None


def unfor_compare_in_widths(widths, offsets, packed, references, members, negate=False, mask=None, combine="new", output=None, check=True):
    """FoR.unfor_compare_in over a mixed-width column: membership in `members` (a member_set result, or anything member_set accepts)
    of the values unfor_pack_widths(widths, offsets, packed, references) yields, inverted by negate=True (NOT IN), joined with the
    mask so far -- combine "new": the hits themselves (`mask` is ignored), "and" / "or": `mask` & hits / `mask` | hits.  `mask` and
    the result are CUDA int32 tensors of 32 words per block (unfor_compare_widths' layout); `output` may be `mask` itself (in place).
    A block whose values all lie outside the set's window, a width-0 block, a block whose `mask` is all zero under "and", and one
    whose `mask` is all ones under "or" are answered without reading their packed bytes.  The per-block device checks of
    unfor_compare_widths, with the same contract: a block that fails them is skipped (its 32 mask words are left as they were);
    `check=True` reads the device error flag back (one sync) and raises, `check=False` stays asynchronous."""
    import torch
    cb = _range_combine(combine, mask)
    if cb and _is_torch(mask) and _is_torch(widths) and mask.numel() != 32 * widths.numel():
        raise ValueError(f"mask holds {mask.numel()} words, expected 32 per block = {32 * widths.numel()}")
    src = _Arg(packed)
    ty = src.ty
    n, lead = _widths_column("unfor_compare_in_widths", src, widths, offsets, references=references)
    m = _select_mask(src, mask, n) if cb else None
    out = _consumer_out(src, output, torch.int32, n * 32, "unfor_compare_in_widths")
    flag = _Flag(check, src.x.device)
    _launch(f"fl_{ty}_unfor_compare_in_widths", src.x.device, *lead, *_member_args(ty, members, src.x.device), int(bool(negate)), cb,
            m.ptr if m is not None and n else None, n, out.data_ptr(), flag.ptr)
    flag.raise_if_set(f"fl_{ty}_unfor_compare_in_widths")       # bitpacking.rs:93,126 unreachable!(); :111-113
    return out


def column_window(ty, widths, references, signed=False, max_bits=1 << 27):
    """(lo, bits) of the smallest NON-CYCLIC window that covers every value a FoR-packed column of element type `ty` can hold: block b
    with reference r and width w holds values in [r, r + 2^w - 1], and the window is [min r, max (r + 2^w - 1)] -- computed from the
    per-block metadata alone (`widths` one u8 per block, `references` one scalar per block or a single one, broadcast), with torch on
    the tensors' device (one sync) or with numpy.  signed=True orders the bit patterns as two's complement, so a column around 0 gets
    a window that starts at a negative value's pattern; `lo` is always the bit pattern unfor_set_build and member sets take.  A block
    whose range passes the end of that order (r + 2^w - 1 > 2^T - 1, or above the largest signed value) has no such window: ValueError
    -- pass an explicit window then.  A window of more than `max_bits` bits (or of more than 2^32) raises ValueError too.  An empty
    column gives (0, 0).
    unfor_set_build with column_window of the PROBE column builds exactly the bits a probe of that column can ever ask for: a key of
    the build side outside it can match no probe row (it is counted in stats[1]), and unfor_compare_in decides every probe block
    against the same window."""
    if ty not in _lib.BITS:
        raise ValueError(f"ty must be one of {list(_lib.TYPES)}")
    T = _lib.BITS[ty]
    if _is_torch(widths) != _is_torch(references):
        raise TypeError("widths and references must both be torch tensors or both be numpy arrays")
    if _is_torch(widths):
        import torch
        if references.device != widths.device:
            raise ValueError(f"tensors live on different devices ({widths.device} vs {references.device})")
        if widths.element_size() != 1 or references.element_size() * 8 != T or references.dtype.is_floating_point:
            raise TypeError(f"widths must be a uint8 tensor and references a {ty} tensor, got {widths.dtype} and {references.dtype}")
        signed_view = {8: torch.int8, 16: torch.int16, 32: torch.int32, 64: torch.int64}[T]
        wv = widths.reshape(-1).view(torch.uint8).to(torch.int64)
        rv = references.contiguous().reshape(-1).view(signed_view).to(torch.int64)
    else:
        wa, ra = np.asarray(widths), np.ascontiguousarray(references)
        if wa.dtype.kind not in "ui" or wa.dtype.itemsize != 1 or ra.dtype.kind not in "ui" or ra.dtype.itemsize * 8 != T:
            raise TypeError(f"widths must be a uint8 array and references a {ty} array, got {wa.dtype} and {ra.dtype}")
        wv, rv = wa.reshape(-1).view(np.uint8).astype(np.int64), ra.reshape(-1).view(f"i{T // 8}").astype(np.int64)
    if len(rv) not in (1, len(wv)):
        raise ValueError("references must hold one scalar per block (or exactly one, broadcast)")
    if len(wv) == 0:
        return 0, 0
    if int(wv.max()) > T:
        raise ValueError(f"column_window: a width above {T}")
    # k: the patterns' rank in the chosen order, held in an int64 -- for T = 64 shifted down by 2^63 (order-preserving)
    sign = 1 << (T - 1)
    if T < 64:
        k = (rv & ((1 << T) - 1)) ^ (sign if signed else 0)
        top, shift = (1 << T) - 1, 0
    else:
        k = rv if signed else rv ^ (-sign)                                 # (-2^63: the sign bit of an int64)
        top, shift = sign - 1, sign
    one = wv * 0 + 1
    span = (one << (wv - (wv == 64) * 1)) - 1                              # 2^w - 1; w = 64 (2^64 - 1) is judged on its own
    full = wv == 64
    wraps = bool(((k > top - span) | (full & (k != -sign))).any())
    if wraps:
        raise ValueError("column_window: a block's range passes the end of the "
                         f"{'signed' if signed else 'unsigned'} order; pass an explicit window (lo, bits)")
    lo_k, hi_k = int(k.min()), top if bool(full.any()) else int((k + span).max())
    bits = hi_k - lo_k + 1
    if bits > max_bits or bits > min(1 << T, 1 << 32):
        raise ValueError(f"column_window: the window holds {bits} bits, more than max_bits = {min(max_bits, 1 << T, 1 << 32)}")
    return ((lo_k + shift) ^ (sign if signed else 0)) & ((1 << T) - 1), bits


def _set_build_target(ty, lo, bits, into, device):
    """The MemberSet a set_build call ORs into: `into` (a device MemberSet of the same ty, lo and bits on `device`) or a fresh, zeroed one"""
    import torch
    T = _lib.BITS[ty]
    lo, bits = int(lo) & ((1 << T) - 1), int(bits)
    if bits < 0 or bits > min(1 << T, 1 << 32):
        raise ValueError(f"bits must lie in [0, {min(1 << T, 1 << 32)}], got {bits}")
    if into is None:
        return MemberSet(ty, lo, bits, torch.zeros((bits + 31) // 32, dtype=torch.int32, device=device))
    if not isinstance(into, MemberSet) or not (_is_torch(into.words) and into.words.is_cuda):
        raise TypeError("into must be a MemberSet whose words live on the device (an earlier unfor_set_build result, or member_set(..., device=...))")
    if into.ty != ty:
        raise TypeError(f"into is a member set of {into.ty}, the column of {ty}")
    if (into.lo, into.bits) != (lo, bits):
        raise ValueError(f"into has the window (lo={into.lo}, bits={into.bits}), the call (lo={lo}, bits={bits})")
    if into.words.device != device:
        raise ValueError(f"tensors live on different devices ({device} vs {into.words.device})")
    if into.words.numel() != (bits + 31) // 32 or into.words.element_size() != 4 or not into.words.is_contiguous():
        raise ValueError(f"into.words must hold {(bits + 31) // 32} contiguous 4-byte words")
    return into


def unfor_set_build_widths(widths, offsets, packed, references, lo, bits, mask=None, into=None, check=True):
    """FoR.unfor_set_build over a mixed-width column: the member set of the values unfor_pack_widths(widths, offsets, packed,
    references) yields where `mask` (32 words per block, unfor_compare_widths' layout; None: everywhere) has a 1, inside the window of
    `bits` bit patterns from `lo` (fl.column_window of the probe column gives the window a probe can ever ask for) -- the build side of
    the semi-join unfor_compare_in probes: `m` of any predicate chain on table A -> unfor_set_build_widths(A's key column, lo, bits,
    mask=m) -> unfor_compare_in_widths(B's key column, set), both key columns packed.  Returns (MemberSet, stats): the set's `words`
    are a CUDA int32 tensor on the column's device, usable in unfor_compare_in* as it stands; stats is a CUDA int64[2] tensor holding
    uint64 bits: kept rows inside the window, kept rows outside it.  `into`: a device MemberSet of the same ty, lo and bits that is
    updated IN PLACE and returned -- the union over several columns or masks (stats counts this call alone).  A block whose mask is
    empty, a block outside the window and a width-0 block are answered without reading their packed bytes.  The per-block device
    checks of unfor_compare_widths: a block that fails them contributes nothing; `check=True` reads the device error flag back (one
    sync) and raises, `check=False` stays asynchronous."""
    import torch
    src = _Arg(packed)
    ty = src.ty
    n, lead = _widths_column("unfor_set_build_widths", src, widths, offsets, references=references)
    m = _select_mask(src, mask, n) if mask is not None else None
    ms = _set_build_target(ty, lo, bits, into, src.x.device)
    stats = torch.zeros(2, dtype=torch.int64, device=src.x.device)
    flag = _Flag(check, src.x.device)
    _launch(f"fl_{ty}_unfor_set_build_widths", src.x.device, *lead, m.ptr if m is not None and n else None, n, _scalar(ty, ms.lo), ms.bits,
            ms.words.data_ptr() if ms.bits else None, stats.data_ptr(), flag.ptr)
    flag.raise_if_set(f"fl_{ty}_unfor_set_build_widths")        # bitpacking.rs:93,126 unreachable!(); :111-113
    return ms, stats


def full_width_column(ty, n_blocks, device):
    """(widths, offsets, references) of a column of `n_blocks` FULL-WIDTH blocks of `ty` on `device`: every width T, block b at byte
    b * 128 * T, one zero reference broadcast to every block.  A full-width bit-packed block is a pure permutation of its 1024 values
    (for u8: the identity), which is the order unfor_lookup* writes -- so with these three a lookup's output drops into any `_widths`
    operator as its packed column: a u8 result as the key column of unfor_aggregate_by_widths, a result of the key's own type as the
    key column of a second lookup."""
    import torch
    if ty not in _lib.BITS:
        raise ValueError(f"ty must be one of {list(_lib.TYPES)}")
    T = _lib.BITS[ty]
    widths = torch.full((int(n_blocks),), T, dtype=torch.uint8, device=device)
    offsets = torch.arange(int(n_blocks), dtype=torch.int64, device=device) * (128 * T)
    references = torch.zeros(1, dtype={"u8": torch.uint8, "u16": torch.uint16, "u32": torch.uint32, "u64": torch.uint64}[ty], device=device)
    return widths, offsets, references


def _present_words(src, lo, n_slots, present):
    """`present` of the lookups: None (every slot is present), or a MemberSet of the key column's type whose window is the table's
    (lo, n_slots) -> its words on the column's device (None for an empty window: nothing is read)"""
    if present is None:
        return None
    ty = src.ty
    T = _lib.BITS[ty]
    if not isinstance(present, MemberSet):
        raise TypeError("present must be a MemberSet (member_set, or an unfor_set_build result)")
    if present.ty != ty:
        raise TypeError(f"present is a member set of {present.ty}, the key column of {ty}")
    if (int(present.lo) & ((1 << T) - 1), present.bits) != (lo, n_slots):
        raise ValueError(f"present has the window (lo={present.lo}, bits={present.bits}), the table (lo={lo}, slots={n_slots})")
    return present.on(src.x.device) if n_slots else None


def _lookup_args(src, n, lo, table, present, missing, mask, hit, output, stats):
    """What both lookup forms share behind the column: the entry's name suffix, the C arguments from `mask` to `stats`, and the three
    tensors the call returns.  `table.dtype` picks the entry: the key's own element size (payload U = T), or one byte (uint8)."""
    import torch
    ty = src.ty
    T = _lib.BITS[ty]
    tb = _Arg(table)
    _same_tier(src, tb)
    if tb.x.dtype.is_floating_point or tb.x.element_size() not in (1, T // 8):
        raise TypeError(f"table must be a {ty} or a uint8 tensor, got {tb.x.dtype}")
    uty = _NP[tb.x.element_size()]
    U = _lib.BITS[uty]
    lo, n_slots = int(lo) & ((1 << T) - 1), tb.n
    if n_slots > min(1 << T, 1 << 32) or n_slots * (U // 8) >= 1 << 31:
        raise ValueError(f"table holds {n_slots} slots of {U // 8} bytes: at most {min(1 << T, 1 << 32)} slots and fewer than 2^31 bytes")
    pr = _present_words(src, lo, n_slots, present)
    m = _select_mask(src, mask, n) if mask is not None else None
    out = _out(tb, output, uty, n * 1024, "unfor_lookup")
    _same_tier(src, out)
    h = _consumer_out(src, hit, torch.int32, n * 32, "unfor_lookup hit")
    if stats is None:
        stats = torch.zeros(2, dtype=torch.int64, device=src.x.device)
    st = _block_words(stats, "stats", 2, 8, src, 1)[0]
    args = (m.ptr if m is not None and n else None, n, _scalar(ty, lo), n_slots, tb.ptr if n_slots else None,
            pr.data_ptr() if pr is not None else None, _scalar(uty, missing), out.ptr if n else None, h.data_ptr() if n else None, st.ptr)
    return ("" if U == T else "_u8"), args, (out.x, h, st.x)


def unfor_lookup_widths(widths, offsets, packed, references, lo, table, present=None, missing=0, mask=None, hit=None, output=None, stats=None,
                        check=True):
    """The probe side of a payload join over a mixed-width key column: for every row `mask` keeps (32 words per block,
    unfor_compare_widths' layout; None: every row) with the key k = unfor_pack_widths(widths, offsets, packed, references)[row] and
    j = (k - lo) mod 2^T, the result is table[j] when j < len(table) and bit j of `present` is set (a MemberSet with the window lo,
    len(table) -- ValueError otherwise; None: every slot is present), `missing` otherwise.  `table` is a CUDA tensor of the key's own
    type or of uint8; its dtype picks the entry point and is the result's.  Returns (column, hit, stats):
      * column: n_blocks * 1024 values, every block in FULL-WIDTH PACKED order -- with fl.full_width_column(ty of the table, ...) the
        packed column of any `_widths` operator (a uint8 column is in row order: the u8 key column of unfor_aggregate_by_widths as it
        stands; BitPacking.unpack(T, column) gives any other back in row order); `output` if given;
      * hit: the hits as a mask of 32 words per block; `hit` if given, and `hit=mask` is the in-place form;
      * stats: a CUDA int64[2] tensor holding uint64 bits, += (hits, kept rows that miss); `stats` if given, else a fresh zeroed one.
    A block whose mask is empty and a block outside the window are all `missing` without a packed load or a gather; a width-0 block
    inside the window takes one table read.  A table of at most 8192 bytes is looked up in LDS, a larger one gathered from device
    memory.  The per-block device checks of unfor_compare_widths: a block that fails them is left untouched (column, hit and stats);
    `check=True` reads the device error flag back (one sync) and raises, `check=False` stays asynchronous."""
    src = _Arg(packed)
    ty = src.ty
    n, lead = _widths_column("unfor_lookup_widths", src, widths, offsets, references=references)
    suffix, args, result = _lookup_args(src, n, lo, table, present, missing, mask, hit, output, stats)
    flag = _Flag(check, src.x.device)
    _launch(f"fl_{ty}_unfor_lookup{suffix}_widths", src.x.device, *lead, *args, flag.ptr)
    flag.raise_if_set(f"fl_{ty}_unfor_lookup{suffix}_widths")   # bitpacking.rs:93,126 unreachable!(); :111-113
    return result


class GroupTable:
    """The table unfor_aggregate_by_window* accumulates into: the key column's element type `ty`, the window (`lo`, `n_groups`) and, for
    slot j = (key - lo) mod 2^T, `counts`, `sums`, `mins`, `maxs`: CUDA int64[n_groups] tensors holding uint64 bits, or None for an
    array the call does not maintain."""
    __slots__ = ("ty", "lo", "n_groups", "counts", "sums", "mins", "maxs")

    def __init__(self, ty, lo, n_groups, counts=None, sums=None, mins=None, maxs=None):
        self.ty, self.lo, self.n_groups, self.counts, self.sums, self.mins, self.maxs = ty, lo, n_groups, counts, sums, mins, maxs

    def __iter__(self):
        return iter((self.ty, self.lo, self.n_groups, self.counts, self.sums, self.mins, self.maxs))

    def __repr__(self):
        return f"GroupTable({self.ty}, lo={self.lo}, n_groups={self.n_groups}, what={self.what()})"

    def what(self):
        """the names of the arrays the table holds, in the order count, sum, min, max"""
        return tuple(name for name, t in zip(_WINDOW_WHAT, (self.counts, self.sums, self.mins, self.maxs)) if t is not None)

    def _pointers(self):
        return tuple(t.data_ptr() if t is not None and self.n_groups else None for t in (self.counts, self.sums, self.mins, self.maxs))


_WINDOW_WHAT = ("count", "sum", "min", "max")


def _window_what(what):
    """`what` of unfor_aggregate_by_window*: a tuple or list of distinct names out of count, sum, min, max -> in that order"""
    if isinstance(what, str) or not isinstance(what, (tuple, list)):
        raise TypeError(f"what must be a tuple of names out of {_WINDOW_WHAT}, got {what!r}")
    if any(w not in _WINDOW_WHAT for w in what) or len(set(what)) != len(what):
        raise ValueError(f"what must hold distinct names out of {_WINDOW_WHAT}, got {tuple(what)!r}")
    return tuple(w for w in _WINDOW_WHAT if w in what)


def _group_table_target(ty, lo, n_groups, names, into, device):
    """The GroupTable a call accumulates into: `into` (the same ty, lo, n_groups and arrays, on `device`) or a fresh one of identities"""
    import torch
    T = _lib.BITS[ty]
    lo, n_groups = int(lo) & ((1 << T) - 1), int(n_groups)
    if n_groups < 0 or n_groups > min(1 << T, 1 << 32):
        raise ValueError(f"n_groups must lie in [0, {min(1 << T, 1 << 32)}], got {n_groups}")
    if into is None:
        fresh = {"count": 0, "sum": 0, "min": -1, "max": 0}                 # (-1: the bits of 2^64 - 1)
        return GroupTable(ty, lo, n_groups, *(torch.full((n_groups,), fresh[w], dtype=torch.int64, device=device) if w in names else None
                                              for w in _WINDOW_WHAT))
    if not isinstance(into, GroupTable):
        raise TypeError("into must be a GroupTable (an earlier unfor_aggregate_by_window result)")
    if (into.ty, into.lo, into.n_groups) != (ty, lo, n_groups):
        raise ValueError(f"into is a table of {into.ty} with the window (lo={into.lo}, n_groups={into.n_groups}), the call of {ty} with "
                         f"(lo={lo}, n_groups={n_groups})")
    if into.what() != names:
        raise ValueError(f"into holds the arrays {into.what()}, the call maintains {names}")
    for t in (into.counts, into.sums, into.mins, into.maxs):
        if t is None:
            continue
        if not (_is_torch(t) and t.is_cuda):
            raise TypeError("into's arrays must be CUDA tensors")
        if t.device != device:
            raise ValueError(f"tensors live on different devices ({device} vs {t.device})")
        if t.numel() != n_groups or t.element_size() != 8 or t.dtype.is_floating_point or not t.is_contiguous():
            raise ValueError(f"into's arrays must hold {n_groups} contiguous 8-byte integers")
    return into


def unfor_aggregate_by_window_widths(widths, offsets, packed, references, key_widths, key_offsets, key_packed, key_references, lo, n_groups,
                                     mask=None, what=("count", "sum"), into=None, check=True):
    """FoR.unfor_aggregate_by_window over two mixed-width columns of one element type and block count: GROUP BY a wide key inside a
    dense window -- SELECT l_orderkey, SUM(l_quantity) ... GROUP BY l_orderkey.  Every row `mask` keeps (32 words per block,
    unfor_compare_widths' layout; None: every row) with the key k = unfor_pack_widths(key_widths, key_offsets, key_packed,
    key_references)[i] updates slot j = (k - lo) mod 2^T of the arrays `what` names ("count", "sum", "min", "max") with the value
    unfor_pack_widths(widths, offsets, packed, references)[i] when j < n_groups, and is counted as outside otherwise; (lo, n_groups)
    of a key column comes from fl.column_window(ty, key_widths, key_references).  Returns (GroupTable, stats): the table's arrays are
    CUDA int64[n_groups] tensors holding uint64 bits (None for what is not named), freshly initialised to the identities 0 / 0 /
    2^64 - 1 / 0; stats is a CUDA int64[2] tensor holding uint64 bits: kept rows inside the window, kept rows outside it.  `into`: a
    GroupTable of the same ty, lo, n_groups and arrays that is updated IN PLACE and returned -- several masks, columns or shards of
    one table (stats counts this call alone).  packed=None (widths, offsets and references are then ignored) is the COUNT-only form:
    the key column stands in both places and what must be ("count",); without "sum", "min" and "max" the value column is never read.
    A block whose mask is empty and a key block outside the window read neither column; a width-0 key block reads no key byte.  The
    per-block device checks of unfor_pack_widths run on BOTH columns: a block that fails either contributes nothing; `check=True`
    reads the device error flag back (one sync) and raises, `check=False` stays asynchronous."""
    import torch
    names = _window_what(what)
    if packed is None:
        if names != ("count",):
            raise ValueError('packed=None is the COUNT-only form: what must be ("count",)')
        widths, offsets, packed, references = key_widths, key_offsets, key_packed, key_references
    src, ksrc = _Arg(packed), _Arg(key_packed)
    ty = src.ty
    if ksrc.ty != ty:
        raise TypeError(f"the key column must have the value column's element type, got {ksrc.ty} and {ty}")
    n, lead = _widths_column("unfor_aggregate_by_window_widths", src, widths, offsets, ksrc, references=references)
    kn, klead = _widths_column("unfor_aggregate_by_window_widths", ksrc, key_widths, key_offsets, src, references=key_references)
    if kn != n:
        raise ValueError(f"the key column holds {kn} blocks, the value column {n}")
    m = _select_mask(src, mask, n) if mask is not None else None
    table = _group_table_target(ty, lo, n_groups, names, into, src.x.device)
    stats = torch.zeros(2, dtype=torch.int64, device=src.x.device)
    flag = _Flag(check, src.x.device)
    _launch(f"fl_{ty}_unfor_aggregate_by_window_widths", src.x.device, *lead, *klead, m.ptr if m is not None and n else None, n,
            _scalar(ty, table.lo), table.n_groups, *table._pointers(), stats.data_ptr(), flag.ptr)
    flag.raise_if_set(f"fl_{ty}_unfor_aggregate_by_window_widths")   # bitpacking.rs:93,126 unreachable!(); :111-113
    return table, stats


def _aggregate_by_lookup_args(name, src, n, lo, table, present, mask, result, stats):
    """What both fused forms share behind the two columns: the C arguments from `mask` to `stats`, and the two tensors the call returns.
    The table is a uint8 tensor (one group code per slot); `present` is checked against its window as unfor_lookup_widths does."""
    import torch
    ty = src.ty
    T = _lib.BITS[ty]
    tb = _Arg(table)
    _same_tier(src, tb)
    if tb.x.dtype != torch.uint8:
        raise TypeError(f"table must be a uint8 tensor (one of 256 group codes per slot), got {tb.x.dtype}")
    lo, n_slots = int(lo) & ((1 << T) - 1), tb.n
    if n_slots > min(1 << T, 1 << 32) or n_slots >= 1 << 31:
        raise ValueError(f"table holds {n_slots} slots: at most {min(1 << T, 1 << 32)} slots and fewer than 2^31 bytes")
    pr = _present_words(src, lo, n_slots, present)
    m = _select_mask(src, mask, n) if mask is not None else None
    dev = src.x.device
    if result is None:
        out = torch.empty((AGGREGATE_BY_GROUPS, 4), dtype=torch.int64, device=dev)
    else:
        out = _consumer_out(src, result, torch.int64, AGGREGATE_BY_GROUPS * 4, name).view(AGGREGATE_BY_GROUPS, 4)
    if stats is None:
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
    st = _block_words(stats, "stats", 2, 8, src, 1)[0]
    args = (m.ptr if m is not None and n else None, n, _scalar(ty, lo), n_slots, tb.ptr if n_slots else None,
            pr.data_ptr() if pr is not None else None, out.data_ptr(), st.ptr)
    return args, (out, st.x)


def unfor_aggregate_by_lookup_widths(widths, offsets, packed, references, key_widths, key_offsets, key_packed, key_references, lo, table,
                                     present=None, mask=None, result=None, stats=None, check=True):
    """GROUP BY a dimension attribute, fused: unfor_lookup_widths with a uint8 table followed by unfor_aggregate_by_widths under the
    hits, in one pass over two mixed-width columns of one element type and block count, with no code column and no hit mask written
    -- SELECT n_name, SUM(revenue) ... GROUP BY n_name through l_suppkey.  Every row `mask` keeps (32 words per block,
    unfor_compare_widths' layout; None: every row) with the key k = unfor_pack_widths(key_widths, key_offsets, key_packed,
    key_references)[i] and j = (k - lo) mod 2^T updates group table[j] with the value unfor_pack_widths(widths, offsets, packed,
    references)[i] when j < len(table) and bit j of `present` is set (a MemberSet with the window lo, len(table) -- ValueError
    otherwise; None: every slot is present), and is counted as a miss otherwise.  `table` is a CUDA uint8 tensor.  Returns
    (result, stats): result is a CUDA int64[256, 4] tensor (`result` if given), row g = count, sum, min, max of group g as
    FoR.unfor_aggregate_by's, every row written by every call; stats is a CUDA int64[2] tensor holding uint64 bits, += (hits, kept rows
    that miss); `stats` if given, else a fresh zeroed one.  A block whose mask is empty reads nothing, a key block outside the window
    reads neither column, a width-0 key block reads no key byte.  The per-block device checks of unfor_pack_widths run on BOTH
    columns: a block that fails either contributes nothing; `check=True` reads the device error flag back (one sync) and raises,
    `check=False` stays asynchronous."""
    src, ksrc = _Arg(packed), _Arg(key_packed)
    ty = src.ty
    if ksrc.ty != ty:
        raise TypeError(f"the key column must have the value column's element type, got {ksrc.ty} and {ty}")
    n, lead = _widths_column("unfor_aggregate_by_lookup_widths", src, widths, offsets, ksrc, references=references)
    kn, klead = _widths_column("unfor_aggregate_by_lookup_widths", ksrc, key_widths, key_offsets, src, references=key_references)
    if kn != n:
        raise ValueError(f"the key column holds {kn} blocks, the value column {n}")
    args, out = _aggregate_by_lookup_args("unfor_aggregate_by_lookup_widths", src, n, lo, table, present, mask, result, stats)
    flag = _Flag(check, src.x.device)
    _launch(f"fl_{ty}_unfor_aggregate_by_lookup_widths", src.x.device, *lead, *klead, *args, flag.ptr)
    flag.raise_if_set(f"fl_{ty}_unfor_aggregate_by_lookup_widths")   # bitpacking.rs:93,126 unreachable!(); :111-113 -- of either column
    return out


def unfor_compare_columns_widths(a_widths, a_offsets, a_packed, a_references, op, b_widths, b_offsets, b_packed, b_references, *,
                                 signed=False, mask=None, combine="new", output=None, check=True):
    """FoR.unfor_compare_columns over two mixed-width columns of the same element type and block count: va <op> vb of the values
    unfor_pack_widths yields for column a and for column b in the same rows (signed=True: of the two's-complement values), joined
    with the mask so far -- combine "new": the hits themselves (`mask` is ignored), "and" / "or": `mask` & hits / `mask` | hits.
    `mask` and the result are CUDA int32 tensors of 32 words per block (unfor_compare_widths' layout); `output` may be `mask` itself
    (in place).  A block pair its references and widths decide, a block whose `mask` is all zero under "and", and one whose `mask`
    is all ones under "or" are answered without reading either column; a block of width 0 is never read.  The per-block device
    checks of unfor_pack_widths run on BOTH columns: a block that fails either is skipped (its 32 mask words are left as they were,
    neither column is read); `check=True` reads the device error flag back (one sync) and raises, `check=False` stays asynchronous."""
    import torch
    cb = _range_combine(combine, mask)
    if cb and _is_torch(mask) and _is_torch(a_widths) and mask.numel() != 32 * a_widths.numel():
        raise ValueError(f"mask holds {mask.numel()} words, expected 32 per block = {32 * a_widths.numel()}")
    sa, sb = _Arg(a_packed), _Arg(b_packed)
    ty = sa.ty
    if sb.ty != ty:
        raise TypeError(f"both columns must have one element type, got {ty} and {sb.ty}")
    n, lead_a = _widths_column("unfor_compare_columns_widths", sa, a_widths, a_offsets, sb, references=a_references)
    nb, lead_b = _widths_column("unfor_compare_columns_widths", sb, b_widths, b_offsets, sa, references=b_references)
    if nb != n:
        raise ValueError(f"column b holds {nb} blocks, column a {n}")
    m = _select_mask(sa, mask, n) if cb else None
    out = _consumer_out(sa, output, torch.int32, n * 32, "unfor_compare_columns_widths")
    flag = _Flag(check, sa.x.device)
    _launch(f"fl_{ty}_unfor_compare_columns_widths", sa.x.device, *lead_a, *lead_b, BitPacking.CMP[op], int(bool(signed)), cb,
            m.ptr if m is not None and n else None, n, out.data_ptr(), flag.ptr)
    flag.raise_if_set(f"fl_{ty}_unfor_compare_columns_widths")  # bitpacking.rs:93,126 unreachable!(); :111-113 -- of either column
    return out


def mask_offsets(mask):
    """Device tier: (out_offsets, total) for a selection mask (a CUDA int32 / uint32 tensor of 32 words per block, as the compare
    functions return) -- out_offsets[b] = number of mask bits set in the blocks before b = where block b's kept values start in
    the compacted output of unfor_select (a CUDA int64 tensor, in elements), total = a 1-element CUDA int64 tensor holding the
    number of kept values.  No host round trip."""
    import torch
    if not _is_torch(mask):
        raise TypeError("mask_offsets is device tier (pass a CUDA int32 tensor)")
    m, n = _block_words(mask, "mask", 32, 4)
    dev = m.x.device
    offsets = torch.empty(n, dtype=torch.int64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    _launch("fl_mask_offsets", dev, m.ptr, n, offsets.data_ptr(), total.data_ptr())
    return offsets, total


def _select_call(name, src, n, lead, mask, out_offsets, total, output, check):
    """The part the two select forms share: mask / out_offsets / output validation, the launch, the error flag.  `lead`: the
    form's own leading C arguments, in front of (mask, out_offsets, out, out_len, n_blocks, err_flag, stream)."""
    import torch
    m = _select_mask(src, mask, n)
    if out_offsets is None:
        out_offsets, total = mask_offsets(m.x)
    oo = _Arg(out_offsets, "u64")
    _same_tier(src, oo)
    if oo.n != n:
        raise ValueError("out_offsets must hold one entry per block")
    dev = src.x.device
    if output is None:
        if total is None:
            raise ValueError("output=None needs `total` (mask_offsets' second result) to size the result")
        out = _Arg(torch.empty(int(total.item()), dtype=src.x.dtype, device=dev), src.ty)   # the one sync
    else:
        out = _Arg(output, src.ty)
        _same_tier(src, out)
    flag = _Flag(check, dev)
    _launch(name, dev, *lead, m.ptr, oo.ptr, out.ptr, out.n, n, flag.ptr)
    flag.raise_if_set(name)                 # a run outside `output`; the mixed form: bitpacking.rs:93,126 unreachable!(); :111-113
    return out.x


def unfor_select_widths(widths, offsets, packed, references, mask, out_offsets=None, total=None, output=None, check=True):
    """FoR.unfor_select over a mixed-width column: the values unfor_pack_widths(widths, offsets, packed, references) yields where
    `mask` (32 words per block, unfor_compare_widths' layout) has a 1, compacted, in column order -- `references` a CUDA tensor of
    one scalar per block (or a single one, broadcast; ONE zero reference selects from a plain bit-packed column).  A block whose
    mask is empty is never read.  `out_offsets` / `total` are mask_offsets(mask)'s results (computed here if not given); with
    `output=None` the total is read back once to size the result (one sync).  The per-block device checks of unfor_pack_widths: a
    block that fails them, or whose run does not fit `output`, is skipped (its output slots are left as they were); `check=True`
    reads the device error flag back (one sync) and raises, `check=False` stays asynchronous."""
    src = _Arg(packed)
    n, lead = _widths_column("unfor_select_widths", src, widths, offsets, references=references)
    return _select_call(f"fl_{src.ty}_unfor_select_widths", src, n, lead, mask, out_offsets, total, output, check)


def aggregate_reduce(block_aggs):
    """Device tier: the combination of per-block aggregates (a CUDA int64 tensor of 4 words per block, as unfor_aggregate returns) --
    counts and sums added (wrapping), the smallest min, the largest max -- as a CUDA int64[4] tensor: count, sum, min, max (uint64 bit
    patterns).  No blocks give the identity (0, 0, 2^64 - 1, 0).  Deterministic; no host round trip."""
    import torch
    if not _is_torch(block_aggs):
        raise TypeError("aggregate_reduce is device tier (pass a CUDA int64 tensor)")
    g, n = _block_words(block_aggs, "block_aggs", 4, 8)
    result = torch.empty(4, dtype=torch.int64, device=g.x.device)
    _launch("fl_aggregate_reduce", g.x.device, g.ptr if n else None, n, result.data_ptr())
    return result


def _aggregate_call(name, src, n, lead, mask, block_aggs, check):
    """The part the two aggregate forms share: mask / block_aggs validation, the two launches, the error flag.  `lead`: the form's
    own leading C arguments, in front of (mask, n_blocks, block_aggs, err_flag, stream)."""
    import torch
    m = _select_mask(src, mask, n) if mask is not None else None
    dev = src.x.device
    if block_aggs is None:
        slots = torch.empty((n, 4), dtype=torch.int64, device=dev)
    else:
        slots = _consumer_out(src, block_aggs, torch.int64, n * 4, name.split("_", 2)[2]).view(n, 4)
    flag = _Flag(check, dev)
    _launch(name, dev, *lead, m.ptr if m is not None and n else None, n, slots.data_ptr() if n else None, flag.ptr)
    result = aggregate_reduce(slots)        # enqueued before the flag is read back: the sync below covers both launches
    flag.raise_if_set(name)                 # the mixed form: bitpacking.rs:93,126 unreachable!(); :111-113
    return result, slots


def unfor_aggregate_widths(widths, offsets, packed, references, mask=None, block_aggs=None, check=True):
    """FoR.unfor_aggregate over a mixed-width column: COUNT / SUM / MIN / MAX of the values unfor_pack_widths(widths, offsets, packed,
    references) yields where `mask` (32 words per block, unfor_compare_widths' layout; None: everywhere) has a 1 -- `references` a CUDA
    tensor of one scalar per block (or a single one, broadcast; ONE zero reference aggregates a plain bit-packed column).  Returns
    (result, block_aggs) as FoR.unfor_aggregate does.  The per-block device checks of unfor_pack_widths: a block that fails them is
    skipped and ITS SLOT HOLDS THE IDENTITY (0, 0, 2^64 - 1, 0), so `result` combines the valid blocks; `check=True` reads the device
    error flag back (one sync) and raises, `check=False` stays asynchronous."""
    src = _Arg(packed)
    n, lead = _widths_column("unfor_aggregate_widths", src, widths, offsets, references=references)
    return _aggregate_call(f"fl_{src.ty}_unfor_aggregate_widths", src, n, lead, mask, block_aggs, check)


def _expr_code(expr):
    """'*', '+', '-' -> fl_expr; anything else is refused here, before a buffer is looked at"""
    if not isinstance(expr, str) or expr not in FoR.EXPR:
        raise ValueError(f"expr must be one of {', '.join(map(repr, FoR.EXPR))}, got {expr!r}")
    return FoR.EXPR[expr]


def unfor_aggregate_columns_widths(a_widths, a_offsets, a_packed, a_references, expr, b_widths, b_offsets, b_packed, b_references,
                                   mask=None, block_aggs=None, check=True):
    """FoR.unfor_aggregate_columns over two mixed-width columns of the same element type and block count: COUNT / SUM / MIN / MAX of
    va `expr` vb ('*', '+', '-'; both values zero-extended to 64 bits first) of the values unfor_pack_widths yields for column a and
    for column b in the same rows, where `mask` (32 words per block, unfor_compare_widths' layout; None: everywhere) has a 1.
    Returns (result, block_aggs) as FoR.unfor_aggregate does.  The per-block device checks of unfor_pack_widths run on BOTH columns:
    a block that fails either is skipped (neither column is read) and ITS SLOT HOLDS THE IDENTITY (0, 0, 2^64 - 1, 0), so `result`
    combines the valid blocks; `check=True` reads the device error flag back (one sync) and raises, `check=False` stays
    asynchronous."""
    ex = _expr_code(expr)
    sa, sb = _Arg(a_packed), _Arg(b_packed)
    if sb.ty != sa.ty:
        raise TypeError(f"both columns must have one element type, got {sa.ty} and {sb.ty}")
    if _numel(b_widths) != _numel(a_widths):
        raise ValueError(f"column b holds {_numel(b_widths)} blocks, column a {_numel(a_widths)}")
    n, lead_a = _widths_column("unfor_aggregate_columns_widths", sa, a_widths, a_offsets, sb, references=a_references)
    _, lead_b = _widths_column("unfor_aggregate_columns_widths", sb, b_widths, b_offsets, sa, references=b_references)
    return _aggregate_call(f"fl_{sa.ty}_unfor_aggregate_columns_widths", sa, n, (ex, *lead_a, *lead_b), mask, block_aggs, check)


AGGREGATE_BY_GROUPS = 256                   # include/fastlanes_amd.h: one slot per possible u8 key


def _aggregate_by_call(name, src, n, lead, mask, result, check):
    """The part the grouped-aggregate forms share: mask / result validation, the launch, the error flag.  `lead`: the form's own
    leading C arguments (`expr` and the value columns', then the key column's), in front of (mask, n_blocks, result, err_flag, stream)."""
    import torch
    m = _select_mask(src, mask, n) if mask is not None else None
    dev = src.x.device
    if result is None:
        out = torch.empty((AGGREGATE_BY_GROUPS, 4), dtype=torch.int64, device=dev)
    else:
        out = _consumer_out(src, result, torch.int64, AGGREGATE_BY_GROUPS * 4, name[name.index("unfor"):]).view(AGGREGATE_BY_GROUPS, 4)
    flag = _Flag(check, dev)
    _launch(name, dev, *lead, m.ptr if m is not None and n else None, n, out.data_ptr(), flag.ptr)
    flag.raise_if_set(name)                 # the mixed form: bitpacking.rs:93,126 unreachable!(); :111-113 -- of any column
    return out


def unfor_aggregate_by_widths(widths, offsets, packed, references, key_widths, key_offsets, key_packed, key_references, mask=None,
                              result=None, check=True):
    """FoR.unfor_aggregate_by over two mixed-width columns of the same block count: COUNT / SUM / MIN / MAX of the values
    unfor_pack_widths(widths, offsets, packed, references) yields, grouped by the u8 keys unfor_pack_widths(key_widths, key_offsets,
    key_packed, key_references) yields in the same rows, where `mask` (32 words per block, unfor_compare_widths' layout; None:
    everywhere) has a 1.  Returns a CUDA int64[256, 4] tensor (`result` if given), row g = count, sum, min, max of key g as
    FoR.unfor_aggregate_by does.  The per-block device checks of unfor_pack_widths run on BOTH columns: a block that fails either
    contributes nothing; `check=True` reads the device error flag back (one sync) and raises, `check=False` stays asynchronous."""
    src, ksrc = _Arg(packed), _Arg(key_packed, "u8")
    n, lead = _widths_column("unfor_aggregate_by_widths", src, widths, offsets, ksrc, references=references)
    kn, klead = _widths_column("unfor_aggregate_by_widths", ksrc, key_widths, key_offsets, src, references=key_references)
    if kn != n:
        raise ValueError(f"the key column holds {kn} blocks, the value column {n}")
    return _aggregate_by_call(f"fl_{src.ty}_unfor_aggregate_by_widths", src, n, (*lead, *klead), mask, result, check)


def unfor_aggregate_by_columns_widths(a_widths, a_offsets, a_packed, a_references, expr, b_widths, b_offsets, b_packed, b_references,
                                      key_widths, key_offsets, key_packed, key_references, mask=None, result=None, check=True):
    """FoR.unfor_aggregate_by_columns over three mixed-width columns of the same block count: COUNT / SUM / MIN / MAX of va `expr` vb
    ('*', '+', '-'; both values zero-extended to 64 bits first) of the values unfor_pack_widths yields for column a and for column b
    (one element type), grouped by the u8 keys unfor_pack_widths(key_widths, key_offsets, key_packed, key_references) yields in the
    same rows, where `mask` (32 words per block, unfor_compare_widths' layout; None: everywhere) has a 1 -- SELECT k, SUM(price *
    discount) WHERE <mask> GROUP BY k.  Returns a CUDA int64[256, 4] tensor (`result` if given), row g = count, sum, min, max of key g
    as FoR.unfor_aggregate_by does.  The per-block device checks of unfor_pack_widths run on ALL THREE columns: a block that fails any
    contributes nothing and none of its columns is read; `check=True` reads the device error flag back (one sync) and raises,
    `check=False` stays asynchronous."""
    ex = _expr_code(expr)
    sa, sb, ksrc = _Arg(a_packed), _Arg(b_packed), _Arg(key_packed, "u8")
    if sb.ty != sa.ty:
        raise TypeError(f"both value columns must have one element type, got {sa.ty} and {sb.ty}")
    if _numel(b_widths) != _numel(a_widths):
        raise ValueError(f"column b holds {_numel(b_widths)} blocks, column a {_numel(a_widths)}")
    if _numel(key_widths) != _numel(a_widths):
        raise ValueError(f"the key column holds {_numel(key_widths)} blocks, the value columns {_numel(a_widths)}")
    n, lead_a = _widths_column("unfor_aggregate_by_columns_widths", sa, a_widths, a_offsets, sb, ksrc, references=a_references)
    _, lead_b = _widths_column("unfor_aggregate_by_columns_widths", sb, b_widths, b_offsets, sa, references=b_references)
    _, klead = _widths_column("unfor_aggregate_by_columns_widths", ksrc, key_widths, key_offsets, sa, references=key_references)
    return _aggregate_by_call(f"fl_{sa.ty}_unfor_aggregate_by_columns_widths", sa, n, (ex, *lead_a, *lead_b, *klead), mask, result, check)


def for_pack_widths(widths, offsets, input, references, output, check=True):
    """`for b: FoR::for_pack::<widths[b]>(&input[b*1024..], references[b], &mut output[offsets[b]..])` (ffor.rs:24-36)."""
    src = _Arg(input)
    ty = src.ty
    out = _Arg(output, ty)
    r, aux = _block_references(src, ty, references, _Arg(widths, "u8").n)
    _widths_call("for_pack_widths", ty, widths, offsets, out, src, check, aux)
    return out.x


def for_widths(mins, maxs):
    """The encoder's step between block_min_max and for_pack_widths: widths[b] = bit length of maxs[b] - mins[b], the
    smallest W for which for_pack::<W>(block b, mins[b]) loses nothing (0 for a constant block).  CUDA tensors in, a CUDA
    uint8 tensor out; asynchronous.  (The reference selects no widths: this is its callers' arithmetic.)"""
    import torch
    lo = _Arg(mins)
    ty = lo.ty
    hi = _Arg(maxs, ty)
    _same_tier(lo, hi)
    if not lo.torch:
        raise TypeError("for_widths is device tier: pass CUDA tensors")
    if hi.n != lo.n:
        raise ValueError("mins and maxs must hold one entry per block")
    widths = torch.empty(lo.n, dtype=torch.uint8, device=lo.x.device)
    _launch(f"fl_{ty}_for_widths", lo.x.device, lo.ptr, hi.ptr, lo.n, widths.data_ptr())
    return widths


def undelta_pack_widths(widths, offsets, packed, base, output=None, check=True, untranspose=False):
    """`for b: Delta::undelta_pack::<widths[b]>(&packed[offsets[b]..], &base[b], ..)` (delta.rs:47-63); the output is in
    transposed order like the reference's, or in ORIGINAL order with `untranspose=True` (the fused extension)."""
    src = _Arg(packed)
    ty = src.ty
    n = _Arg(widths, "u8").n
    b, aux = _block_bases(src, ty, base, n)
    method = "undelta_pack_untranspose_widths" if untranspose else "undelta_pack_widths"
    out = _out(src, output, ty, n * 1024, method)
    _widths_call(method, ty, widths, offsets, src, out, check, aux)
    return out.x


def undelta_compare_range_widths(widths, offsets, packed, base, lo, hi, mask=None, combine="new", output=None, check=True):
    """Delta.undelta_compare_range over a mixed-width column: the cyclic interval [lo, hi] (mod 2^T; predicate_interval gives a
    comparison's) over the values undelta_pack_widths(widths, offsets, packed, base, untranspose=True) yields, joined with the mask so
    far exactly as unfor_compare_range_widths joins it -- the same masks (32 words per block, bit i = original row i), the same
    `combine` names, `output` may be `mask` itself.  A block its bases and width decide, a width-0 block and a block its `mask` already
    decides read no packed byte.  The per-block device checks of unfor_compare_widths, with the same contract: a block that fails them
    is skipped (its 32 mask words are left as they were); `check=True` reads the device error flag back (one sync) and raises,
    `check=False` stays asynchronous."""
    import torch
    cb = _range_combine(combine, mask)
    if cb and _is_torch(mask) and _is_torch(widths) and mask.numel() != 32 * widths.numel():
        raise ValueError(f"mask holds {mask.numel()} words, expected 32 per block = {32 * widths.numel()}")
    src = _Arg(packed)
    ty = src.ty
    n, lead = _widths_column("undelta_compare_range_widths", src, widths, offsets)
    b, aux = _block_bases(src, ty, base, n)
    m = _select_mask(src, mask, n) if cb else None
    out = _consumer_out(src, output, torch.int32, n * 32, "undelta_compare_range_widths")
    flag = _Flag(check, src.x.device)
    _launch(f"fl_{ty}_undelta_compare_range_widths", src.x.device, *lead, *aux, _scalar(ty, lo), _scalar(ty, hi), cb,
            m.ptr if m is not None and n else None, n, out.data_ptr(), flag.ptr)
    flag.raise_if_set(f"fl_{ty}_undelta_compare_range_widths")  # bitpacking.rs:93,126 unreachable!(); :111-113
    return out


def undelta_aggregate_widths(widths, offsets, packed, base, mask=None, block_aggs=None, check=True):
    """Delta.undelta_aggregate over a mixed-width column: COUNT / SUM / MIN / MAX of the values undelta_pack_widths(widths, offsets, packed,
    base, untranspose=True) yields where `mask` (32 words per block, bit i = original row i; None: everywhere) has a 1.  Returns (result,
    block_aggs) as FoR.unfor_aggregate does; the mask of undelta_compare_range_widths chains straight into it.  The per-block device
    checks of unfor_pack_widths, with unfor_aggregate_widths' contract: a block that fails them is skipped and ITS SLOT HOLDS THE IDENTITY
    (0, 0, 2^64 - 1, 0), so `result` combines the valid blocks; `check=True` reads the device error flag back (one sync) and raises,
    `check=False` stays asynchronous."""
    src = _Arg(packed)
    ty = src.ty
    n, lead = _widths_column("undelta_aggregate_widths", src, widths, offsets)
    b, aux = _block_bases(src, ty, base, n)
    return _aggregate_call(f"fl_{ty}_undelta_aggregate_widths", src, n, (*lead, *aux), mask, block_aggs, check)


def undelta_select_widths(widths, offsets, packed, base, mask, out_offsets=None, total=None, output=None, check=True):
    """Delta.undelta_select over a mixed-width column: the values undelta_pack_widths(widths, offsets, packed, base, untranspose=True)
    yields where `mask` (32 words per block, bit i = original row i) has a 1, compacted, in row order; the mask of
    undelta_compare_range_widths chains straight into it.  `out_offsets` / `total` / `output` as unfor_select_widths takes them.  The
    per-block device checks of unfor_pack_widths, with unfor_select_widths' contract: a block that fails them, or whose run does not fit
    `output`, is skipped (its output slots are left as they were); `check=True` reads the device error flag back (one sync) and raises,
    `check=False` stays asynchronous."""
    src = _Arg(packed)
    ty = src.ty
    n, lead = _widths_column("undelta_select_widths", src, widths, offsets)
    b, aux = _block_bases(src, ty, base, n)
    return _select_call(f"fl_{ty}_undelta_select_widths", src, n, (*lead, *aux), mask, out_offsets, total, output, check)


def transpose_delta_pack_widths(widths, offsets, input, base, output, check=True):
    """`for b: pack::<widths[b]>(delta(transpose(&input[b*1024..]), &base[b]))` into output[offsets[b]..] -- the fused encode
    extension (delta.rs:88-95 composed) over per-block widths."""
    src = _Arg(input)
    ty = src.ty
    out = _Arg(output, ty)
    b, aux = _block_bases(src, ty, base, _Arg(widths, "u8").n)
    _widths_call("transpose_delta_pack_widths", ty, widths, offsets, out, src, check, aux)
    return out.x


def unpack_single_widths(widths, offsets, packed, index):
    """`T::unchecked_unpack_single(widths[b], &packed[offsets[b]..], i)` (bitpacking.rs:58,181-200) batched over a mixed-width
    column: `index` is a CUDA int64/uint64 tensor of column-global element indices (block*1024 + i); returns the values.
    An index past the column raises like the reference's assert (bitpacking.rs:152), a width > T like its unreachable!()."""
    src = _Arg(packed)
    n, lead = _widths_column("unpack_single_widths", src, widths, offsets)
    return _single_call(f"fl_{src.ty}_unpack_single_widths", src, index, *lead, n)


class Batch:
    """Many small arrays decoded / encoded in ONE launch (fl_<ty>_unpack_batch / _pack_batch): the shape of a columnar
    engine's chunks -- Vortex keeps 64 Ki values (64 blocks) per chunk and loops `unchecked_unpack` over each
    (bitpacking.rs:109-129), which is launch-bound as one call per chunk.  `packed[a]` / `unpacked[a]` are CUDA tensors of one
    element type on one device (array a: n_blocks[a] blocks of width widths[a]); the constructor uploads the four per-array
    device arrays (pointers, widths, block counts) once, unpack() / pack() are then one asynchronous launch each."""

    def __init__(self, packed, unpacked, widths, references=None, bases=None):
        """`references` (optional): one FoR reference per array -- unpack() / pack() then run unfor_pack::<W> / for_pack::<W>
        (ffor.rs:24-50) on every block of array a with references[a].
        `bases` (optional): one CUDA tensor per array holding its Delta bases, LANES elements per block (delta.rs:7) -- for
        undelta_pack() / transpose_delta_pack()."""
        import torch
        if not (len(packed) == len(unpacked) == len(widths)):
            raise ValueError("packed, unpacked and widths must have one entry per array")
        self.n = len(widths)
        args_p = [_Arg(t) for t in packed]
        args_u = [_Arg(t) for t in unpacked]
        if self.n == 0:
            raise ValueError("an empty batch has no element type")
        self.ty = args_u[0].ty
        T = _lib.BITS[self.ty]
        w = np.asarray(list(widths), dtype=np.int64)
        if (w < 0).any() or (w > T).any():
            raise FastLanesError(1, f"fl_{self.ty}_unpack_batch")      # bitpacking.rs:93,126 unreachable!()
        nb = []
        for a, (p, u) in enumerate(zip(args_p, args_u)):
            if p.ty != self.ty or u.ty != self.ty or not p.torch:
                raise TypeError("all arrays of a batch are CUDA tensors of one element type")
            _same_tier(args_u[0], p, u)
            if u.n % 1024:
                raise ValueError(f"array {a}: the unpacked array must hold 1024 elements per block")
            if p.n != (u.n // 1024) * packed_len(self.ty, int(w[a])):
                raise ValueError(f"array {a}: packed length {p.n} does not match {u.n // 1024} blocks of width {int(w[a])}")
            # the kernel can only SKIP a misaligned array and raise FL_DEVERR_ALIGN (the pointers reach it through HBM), which a
            # caller running with check=False would never see: here, where the pointers are still on the host, it is an error like
            # at every other entry point (FL_ERR_ALIGN).  A width-0 array has no packed bytes: any pointer, or none, will do.
            if u.ptr % 16 or (int(w[a]) != 0 and u.n and p.ptr % 16):
                raise FastLanesError(4, f"fl_{self.ty}_unpack_batch (array {a}: device pointers must be 16-byte aligned)")
            nb.append(u.n // 1024)
        self.device = args_u[0].x.device
        self._keep = (list(packed), list(unpacked))                     # the pointer arrays below refer to these
        up = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)).to(self.device)
        self.d_packed = up([a.ptr for a in args_p], np.int64)
        self.d_unpacked = up([a.ptr for a in args_u], np.int64)
        self.d_widths = up(w, np.uint8)
        self.d_n_blocks = up(nb, np.int32)
        self.max_blocks = max(nb)
        self.d_refs = None
        if references is not None:
            r = [_scalar(self.ty, x).value for x in references]        # python ints: a u64 reference may exceed int64
            if len(r) != self.n:
                raise ValueError("references must hold one entry per array")
            self.d_refs = up(np.array(r, dtype=np.uint64).astype(_NP_DTYPE[self.ty]).view(np.uint8), np.uint8)
        self.unpacked = list(unpacked)
        self.packed = list(packed)
        self.d_bases = None
        if bases is not None:
            if len(bases) != self.n:
                raise ValueError("bases must hold one tensor per array")
            args_b = [_Arg(t, self.ty) for t in bases]
            for a, bb in enumerate(args_b):
                _same_tier(args_u[0], bb)
                if bb.n != nb[a] * (1024 // T):
                    raise ValueError(f"array {a}: bases must hold LANES elements per block")
                if nb[a] and bb.ptr % 16:
                    raise FastLanesError(4, f"fl_{self.ty}_undelta_pack_batch (array {a}: device pointers must be 16-byte aligned)")
            self._keep += (list(bases),)
            self.d_bases = up([a.ptr for a in args_b], np.int64)

    def _run(self, method, first, second, check, delta=False, extra=()):
        """One launch over the batch.  The C argument order is (in, [bases], out, widths, [references], n_blocks, n_arrays, max_blocks,
        [extra], err_flag, stream): Delta's per-array bases sit between the two sides, FoR's references after the widths."""
        if delta:
            if self.d_bases is None:
                raise ValueError("this batch was built without bases")
            data = (first.data_ptr(), self.d_bases.data_ptr(), second.data_ptr(), self.d_widths.data_ptr())
        elif self.d_refs is not None:
            method = {"unpack_batch": "unfor_pack_batch", "pack_batch": "for_pack_batch"}[method]
            data = (first.data_ptr(), second.data_ptr(), self.d_widths.data_ptr(), self.d_refs.data_ptr())
        else:
            data = (first.data_ptr(), second.data_ptr(), self.d_widths.data_ptr())
        flag = _Flag(check, self.device)
        _launch(f"fl_{self.ty}_{method}", self.device, *data, self.d_n_blocks.data_ptr(), self.n, self.max_blocks, *extra, flag.ptr)
        flag.raise_if_set(f"fl_{self.ty}_{method}")

    def undelta_pack(self, untranspose=False, check=False):
        """Delta::undelta_pack::<widths[a]> (delta.rs:47-63) on every block of every array with its bases; the output is in
        transposed order like the reference's, or in ORIGINAL order with `untranspose=True` (the fused extension)."""
        self._run("undelta_pack_batch", self.d_packed, self.d_unpacked, check, delta=True, extra=(1 if untranspose else 0,))
        return self.unpacked

    def transpose_delta_pack(self, check=False):
        """The fused encode pack::<widths[a]>(delta(transpose(unpacked[a]), bases[a])) for every array."""
        self._run("transpose_delta_pack_batch", self.d_unpacked, self.d_packed, check, delta=True)
        return self.packed

    def unpack(self, check=False):
        """packed[a] -> unpacked[a] for every array; returns the list of unpacked tensors."""
        self._run("unpack_batch", self.d_packed, self.d_unpacked, check)
        return self.unpacked

    def pack(self, check=False):
        """unpacked[a] -> packed[a] for every array; returns the list of packed tensors."""
        self._run("pack_batch", self.d_unpacked, self.d_packed, check)
        return self.packed


class MixedWidthPlan:
    """A column whose blocks each have their own width (BASELINE.json config 5): the
    reference's caller loop `for b: T::unchecked_unpack(widths[b], ..)` (bitpacking.rs:109-129)
    as one call.  Built from the host `widths` array: uploads them and prefix-sums the packed byte
    offsets (128*widths[b], back to back) ON THE DEVICE; `widths` / `offsets` are then device arrays
    (see unpack_widths / pack_widths for callers whose widths already live in HBM)."""

    def __init__(self, ty, widths, device=None):
        import torch
        self.ty = ty
        w = _check_widths_host(ty, widths)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("a MixedWidthPlan lives on a GPU")
        if self.device.index is None:        # torch.device('cuda') != torch.device('cuda:0'): pin the index now
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._plan = ctypes.c_void_p()
        lib = _lib.load()
        _launch("fl_mixed_plan_create", self.device, _lib.BITS[ty], w.ctypes.data, w.size, ctypes.byref(self._plan), stream=False)
        self.n_blocks = int(lib.fl_mixed_plan_n_blocks(self._plan))
        self.packed_bytes = int(lib.fl_mixed_plan_packed_bytes(self._plan))

    def close(self):
        if getattr(self, "_plan", None):
            _lib.load().fl_mixed_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: the library may already be gone
            pass

    def _torch_dtype(self):
        import torch
        return {"u8": torch.uint8, "u16": torch.uint16, "u32": torch.uint32, "u64": torch.uint64}[self.ty]

    def _on_device(self, *args):
        for a in args:
            if not a.torch or a.x.device != self.device:
                raise ValueError(f"this plan lives on {self.device}: pass CUDA tensors of that device")

    def _run(self, method, input, n_in, bad_in, output, n_out, bad_out):
        """Either direction over the plan: `input` of exactly n_in elements into `output` (a fresh tensor if None) of exactly n_out."""
        import torch
        src = _Arg(input, self.ty)
        if src.n != n_in:
            raise ValueError(bad_in)
        out = _Arg(output if output is not None else torch.empty(n_out, dtype=self._torch_dtype(), device=self.device), self.ty)
        if out.n != n_out:
            raise ValueError(bad_out)
        self._on_device(src, out)
        _launch(f"fl_{self.ty}_{method}", self.device, self._plan, src.ptr, out.ptr)
        return out.x

    def _packed_len(self):
        return self.packed_bytes // (_lib.BITS[self.ty] // 8)

    def unpack(self, packed, output=None):
        return self._run("unpack_mixed", packed, self._packed_len(), "packed column has the wrong size for this plan",
                         output, self.n_blocks * 1024, "Output buffer must be of size 1024 per block")

    def pack(self, input, output=None):
        return self._run("pack_mixed", input, self.n_blocks * 1024, "Input buffer must be of size 1024 per block",
                         output, self._packed_len(), "packed column has the wrong size for this plan")
