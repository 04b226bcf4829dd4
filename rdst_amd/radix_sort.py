"""Host mirror of rdst's entry points for the device route.

Reference surface (paths in the reference tree):
  * ``RadixSort::radix_sort_unstable`` / ``radix_sort_builder``   src/radix_sort.rs:4-45
  * ``RadixSortBuilder`` and its ``with_*`` methods / ``sort``     src/radix_sort_builder.rs:8-158
  * ``RadixKey`` built-in mappings -> (kind, elem_bytes, levels)   src/radix_key_impl.rs:1-185

Accepted containers: a C-contiguous 1-D ``numpy.ndarray`` (host slice -> ``rdst_hip_sort``)
or a contiguous 1-D ``torch.Tensor`` on a HIP device (device slice ->
``rdst_hip_sort_device``; PyTorch only provides the memory and the stream).  Sorting is in
place, returns ``None`` like the reference, and raises instead of falling back when the
device path is unavailable: this package ships the device route only — the CPU algorithms
remain the reference crate's own.
"""
import ctypes

import numpy as np

from . import _lib
from .tuner import Algorithm, GpuTuner, LowMemoryTuner, SingleThreadedTuner, StandardTuner, Tuner, TuningParams

# dtype name -> (rdst_key_kind, elem_bytes); LEVELS == elem_bytes for every built-in type
_KEY_TABLE = {
    "uint8": (_lib.RDST_KEY_UNSIGNED, 1),
    "uint16": (_lib.RDST_KEY_UNSIGNED, 2),
    "int8": (_lib.RDST_KEY_SIGNED, 1),
    "int16": (_lib.RDST_KEY_SIGNED, 2),
    "uint32": (_lib.RDST_KEY_UNSIGNED, 4),
    "uint64": (_lib.RDST_KEY_UNSIGNED, 8),
    "int32": (_lib.RDST_KEY_SIGNED, 4),
    "int64": (_lib.RDST_KEY_SIGNED, 8),
    "float32": (_lib.RDST_KEY_FLOAT, 4),
    "float64": (_lib.RDST_KEY_FLOAT, 8),
    # no numpy / torch dtype exists for these: pass key="u128" / "i128" with a container of shape
    # (n, 2) whose rows are the little-endian 64-bit limbs [low, high] of one key
    "u128": (_lib.RDST_KEY_UNSIGNED, 16),
    "i128": (_lib.RDST_KEY_SIGNED, 16),
}


def key_info(dtype_name: str):
    """(kind, elem_bytes, levels) of a built-in RadixKey (src/radix_key_impl.rs)."""
    name = str(dtype_name).replace("torch.", "")
    if name not in _KEY_TABLE:
        raise TypeError(f"no device RadixKey mapping for dtype {dtype_name}; supported: {sorted(_KEY_TABLE)}")
    kind, nbytes = _KEY_TABLE[name]
    return kind, nbytes, nbytes


def _is_torch_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _wide(key):
    return key in ("u128", "i128")


def _check_wide_shape(shape, itemsize):
    if len(shape) != 2 or shape[1] * itemsize != 16:
        raise ValueError("a 128-bit key container has shape (n, 2) with 8-byte limbs [low, high]")


def _check_bytes_rows(shape, dtype_ok):
    if len(shape) != 2 or not dtype_ok or not 1 <= shape[1] <= _lib.RDST_BYTES_MAX_N:
        raise ValueError(f"[u8; N] keys: a uint8 container of shape (n, N) with N in 1..{_lib.RDST_BYTES_MAX_N}")


# ---- what every tensor wrapper is made of: checked operands -> buffers -> one call ----

def _current_stream(device=None):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _stream_handle(tensor):
    return _current_stream(tensor.device)


def _ptr(t, empty_is_null=False):
    return ctypes.c_void_p(t.data_ptr() if t is not None and (t.numel() or not empty_is_null) else None)


def _on_device(name, t):
    if not t.is_cuda:
        raise ValueError(f"{name} needs a tensor on a HIP device")


def _keys_operand(name, keys, key=None):
    """the keys of a tensor wrapper, checked: (kind, nbytes, levels, n, per_key)"""
    _on_device(name, keys)
    if _wide(key):
        _check_wide_shape(tuple(keys.shape), keys.element_size())
    if keys.dim() != (2 if _wide(key) else 1) or not keys.is_contiguous():
        raise ValueError("keys must be a contiguous 1-D tensor (rdst sorts a slice)")
    kind, nbytes, levels = key_info(key if key else keys.dtype)
    n = keys.numel() * keys.element_size() // nbytes
    return kind, nbytes, levels, n, (keys.numel() // n if n else 1)   # per_key: container elements per key (2 for the 128-bit limbs)


def _mismatch(t, like):
    """a tmp (tmp_values) tensor that cannot stand in for `like`, whatever its length"""
    return t.dtype != like.dtype or not t.is_contiguous() or t.device != like.device


def _scratch(scratch, need, device, whose="keys"):
    """(scratch, its bytes) for an entry that asks for `need` bytes: the caller's tensor, checked, or a fresh one"""
    import torch
    if scratch is None:
        return torch.empty(max(need, 1), dtype=torch.uint8, device=device), need   # the caching allocator hands out 512-byte aligned blocks
    if scratch.device != device or not scratch.is_contiguous() or scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"scratch must be a contiguous tensor on the {whose}' device with at least {need} bytes")
    return scratch, scratch.numel() * scratch.element_size()


def _call(tensor, check, entry, *args):
    """the tail of a tensor wrapper: `entry(*args, stream)` on the tensor's device and current stream, then, with `check`, the
    blocking look at the status; the blocking hooks, which wait inside `entry`, pass check=False"""
    import torch
    lib = _lib.load()
    with torch.cuda.device(tensor.device):
        s = _stream_handle(tensor)
        _lib.check(getattr(lib, entry)(*args, s))
        if check:
            _lib.check(lib.rdst_hip_device_status(s))


_WHOLE = object()   # the `length` of the plain wrappers: no device-resident length, all keys are sorted
_LENGTH_DTYPES = {"int32": 4, "uint32": 4, "int64": 8, "uint64": 8}


def _device_length(length, keys):
    """the (pointer, len_bytes) arguments of a device-resident length, checked without looking at its value; none for _WHOLE"""
    if length is _WHOLE:
        return ()
    name = str(getattr(length, "dtype", None)).replace("torch.", "")
    if not _is_torch_tensor(length) or name not in _LENGTH_DTYPES or length.numel() != 1 or not length.is_contiguous():
        raise ValueError("length must be a contiguous one-element tensor of dtype int32, int64, uint32 or uint64")
    if length.device != keys.device:
        raise ValueError("length must live on the keys' device")
    return _ptr(length), _LENGTH_DTYPES[name]


def _sort_keys(name, keys, length, tmp, check, key):
    """sort_device_tensor (length: _WHOLE) and sort_device_devlen_tensor"""
    import torch
    kind, nbytes, levels, n, _per_key = _keys_operand(name, keys, key)
    devlen = _device_length(length, keys)
    if n <= 1:
        return
    if tmp is None:
        tmp = torch.empty_like(keys)
    elif _mismatch(tmp, keys) or tmp.numel() < keys.numel():
        raise ValueError("tmp must be a contiguous tensor of the same dtype/device with at least len elements")
    _call(keys, check, "rdst_hip_sort_device_devlen" if devlen else "rdst_hip_sort_device", _ptr(keys), _ptr(tmp), n, *devlen, nbytes, kind, levels)


def sort_device_tensor(keys, tmp=None, check=True, key=None):
    """``rdst_hip_sort_device`` on a 1-D contiguous HIP tensor (``key="u128"/"i128"``: shape (n, 2)).  ``tmp``: optional scratch
    tensor of the same shape/dtype (allocated when omitted).  With ``check`` the call blocks
    and raises if a kernel reported failure; without it the sort stays asynchronous on the
    tensor's current stream (call :func:`device_status` later)."""
    _sort_keys("sort_device_tensor", keys, _WHOLE, tmp, check, key)


def sort_device_devlen_tensor(keys, length, tmp=None, check=True, key=None):
    """``rdst_hip_sort_device_devlen``: :func:`sort_device_tensor` over the first ``m`` keys, where ``m`` is the value of
    ``length`` — a one-element contiguous tensor on the keys' device (int32, int64, uint32 or uint64, read as unsigned) that is
    read on the stream, never by the host: the kernel that produces it may still be running.  The capacity is the number of
    keys (``key="u128"/"i128"``: rows); keys from ``m`` on are not touched.  ``m`` past the capacity changes nothing and
    raises in :func:`device_status` (error bit 32).  The call only enqueues work on the tensor's current stream;
    ``check=False`` makes no blocking call at all."""
    _sort_keys("sort_device_devlen_tensor", keys, length, tmp, check, key)


def sort_bytes_device_tensor(rows, scratch=None, check=True):
    """``rdst_hip_sort_bytes_device``: sort the rows of a contiguous (n, N) uint8 HIP tensor in place, each row one
    ``[u8; N]`` key (src/radix_key_impl.rs:78-85: lexicographic order).  The row base needs no alignment.  ``scratch``:
    optional uint8 HIP tensor of at least ``rdst_hip_sort_bytes_scratch_bytes(n, N)`` bytes (allocated when omitted).  Runs on
    the tensor's current stream; N > 16 blocks (the tie counts come to the host), N <= 16 stays asynchronous unless
    ``check``."""
    _sort_bytes_rows("sort_bytes_device_tensor", "rdst_hip_sort_bytes_device", rows, scratch, check)


def sort_bytes_device_nowait_tensor(rows, scratch=None, check=True):
    """``rdst_hip_sort_bytes_device_nowait``: :func:`sort_bytes_device_tensor` without the host in the loop, for N up to
    ``RDST_BYTES_NOWAIT_MAX_N`` (128); the same arguments, the same scratch size and, bit for bit, the same result.  The
    call only enqueues work on the tensor's current stream; ``check=False`` makes no blocking call at all (kernel failures
    then surface in :func:`device_status`)."""
    _sort_bytes_rows("sort_bytes_device_nowait_tensor", "rdst_hip_sort_bytes_device_nowait", rows, scratch, check)


def _sort_bytes_rows(name, entry, rows, scratch, check):
    import torch
    _on_device(name, rows)
    _check_bytes_rows(tuple(rows.shape), rows.dtype == torch.uint8)
    if not rows.is_contiguous():
        raise ValueError("rows must be a contiguous (n, N) tensor")
    n, n_bytes = int(rows.shape[0]), int(rows.shape[1])
    if n <= 1:
        return
    scratch, sbytes = _scratch(scratch, int(_lib.load().rdst_hip_sort_bytes_scratch_bytes(n, n_bytes)), rows.device, "rows")
    _call(rows, check, entry, _ptr(rows), n, n_bytes, _ptr(scratch), sbytes)


def _sort_pairs(keys, values, length, tmp_keys, tmp_values, check):
    """sort_pairs_device_tensor (length: _WHOLE) and sort_pairs_device_devlen_tensor"""
    import torch
    if not (keys.is_cuda and values.is_cuda) or keys.device != values.device:
        raise ValueError("keys and values must live on the same HIP device")
    if keys.dim() != 1 or values.dim() != 1 or keys.numel() != values.numel():
        raise ValueError("keys and values must be 1-D tensors of the same length")
    if not (keys.is_contiguous() and values.is_contiguous()):
        raise ValueError("keys and values must be contiguous")
    kind, nbytes, levels = key_info(keys.dtype)
    vbytes = values.element_size()
    devlen = _device_length(length, keys)
    n = keys.numel()
    if n <= 1:
        return
    tmp_keys = torch.empty_like(keys) if tmp_keys is None else tmp_keys
    tmp_values = torch.empty_like(values) if tmp_values is None else tmp_values
    for t, ref in ((tmp_keys, keys), (tmp_values, values)):
        if _mismatch(t, ref) or t.numel() < n:
            raise ValueError("tmp tensors must match their originals in dtype, device and length")
    _call(keys, check, "rdst_hip_sort_pairs_device_devlen" if devlen else "rdst_hip_sort_pairs_device", _ptr(keys), _ptr(values), _ptr(tmp_keys),
          _ptr(tmp_values), n, *devlen, nbytes, kind, levels, vbytes)


def sort_pairs_device_tensor(keys, values, tmp_keys=None, tmp_values=None, check=True):
    """``rdst_hip_sort_pairs_device``: sort the 1-D HIP tensor ``keys`` (4- or 8-byte built-in key type) in place
    and permute ``values`` (4- or 8-byte elements, same length) with it.  Stable: equal keys keep their
    input order (rdst promises none, src/radix_sort.rs:21-45)."""
    _sort_pairs(keys, values, _WHOLE, tmp_keys, tmp_values, check)


def sort_pairs_device_devlen_tensor(keys, values, length, tmp_keys=None, tmp_values=None, check=True):
    """``rdst_hip_sort_pairs_device_devlen``: :func:`sort_pairs_device_tensor` over the first ``m`` pairs, ``m`` being the
    value of the device-resident ``length`` (see :func:`sort_device_devlen_tensor`); the capacity is ``keys.numel()``.
    Stable; keys and values from ``m`` on are not touched."""
    _sort_pairs(keys, values, length, tmp_keys, tmp_values, check)


def _index_bytes(index):
    import torch
    if index not in (None, torch.int32, torch.int64):
        raise ValueError("index must be None, torch.int32 or torch.int64")
    return 0 if index is None else (4 if index == torch.int32 else 8)


def topk_limits(dtype, index_bytes=0):
    """``rdst_hip_topk_limits``: (digit_bits, default cand_capacity, most levels a call can take) of the partial sort for keys
    of ``dtype`` (a numpy / torch dtype or its name, ``"u128"`` / ``"i128"``); ``index_bytes``: 0 = keys only, 4 or 8."""
    _kind, nbytes, _levels = key_info(dtype)
    out = (ctypes.c_uint32 * 3)()
    _lib.check(_lib.load().rdst_hip_topk_limits(nbytes, int(index_bytes), out))
    return int(out[0]), int(out[1]), int(out[2])


def topk_scratch_bytes(n, k, dtype, index_bytes=0, cand_capacity=0):
    """``rdst_hip_topk_scratch_bytes``: bytes of scratch :func:`topk_device_tensor` needs for ``k`` of ``n`` keys of ``dtype``
    (0 for widths the entry is not built for)."""
    _kind, nbytes, _levels = key_info(dtype)
    return int(_lib.load().rdst_hip_topk_scratch_bytes(int(n), int(k), nbytes, int(index_bytes), int(cand_capacity)))


def topk_state(scratch):
    """``rdst_hip_debug_topk_state`` (test hook, blocking): what the most recent :func:`topk_device_tensor` on ``scratch``
    decided — dict with ``levels`` (select levels the device used), ``c_below`` (keys strictly before the threshold prefix),
    ``candidates`` (collected) and ``special`` (the keys-only fill or a position digit was reached)."""
    import torch
    out = (ctypes.c_uint64 * 4)()
    with torch.cuda.device(scratch.device):
        _lib.check(_lib.load().rdst_hip_debug_topk_state(_ptr(scratch), _stream_handle(scratch), out))   # (the stream is not its last argument)
    return {"levels": int(out[0]), "c_below": int(out[1]), "candidates": int(out[2]), "special": int(out[3])}


def topk_device_tensor(keys, k, largest=False, index=None, scratch=None, cand_capacity=0, check=True, key=None):
    """``rdst_hip_topk_device``: the ``k`` keys of the 1-D contiguous HIP tensor ``keys`` (``key="u128"/"i128"``: shape (n, 2))
    that come first in the sort's order — ``largest``: last, in descending order —, in that order, as a new tensor; ``keys`` is
    not modified.  ``index``: ``None`` for keys only, ``torch.int32`` or ``torch.int64`` to get the input position of every
    output key as well (4- and 8-byte keys); equal keys appear in ascending position and the lowest positions win a tie at
    the k-th key, so the pair is the first ``k`` of a stable argsort.  ``scratch``: optional uint8 HIP tensor of at least
    :func:`topk_scratch_bytes` bytes (allocated when omitted); ``cand_capacity``: 0 = the library's default, any value >= 1
    gives the same result.  Returns ``(out_keys, out_index or None)``.  The call only enqueues work on the tensor's current
    stream; ``check=False`` makes no blocking call at all (kernel failures then surface in :func:`device_status`)."""
    import torch
    kind, nbytes, levels, n, _per_key = _keys_operand("topk_device_tensor", keys, key)
    k = int(k)
    if not 0 <= k <= n:
        raise ValueError("k must lie in 0..len")
    index_bytes = _index_bytes(index)
    out_keys = torch.empty((k, 2) if _wide(key) else (k,), dtype=keys.dtype, device=keys.device)
    out_index = None if index is None else torch.empty(k, dtype=index, device=keys.device)
    if k == 0:
        return out_keys, out_index
    need = int(_lib.load().rdst_hip_topk_scratch_bytes(n, k, nbytes, index_bytes, int(cand_capacity)))
    scratch, sbytes = _scratch(scratch, need, keys.device)
    _call(keys, check, "rdst_hip_topk_device", _ptr(keys), n, k, _ptr(out_keys), _ptr(out_index), index_bytes, _ptr(scratch), sbytes,
          int(cand_capacity), nbytes, kind, levels, _lib.RDST_TOPK_LARGEST if largest else 0)
    return out_keys, out_index


def select_limits(dtype, index_bytes=0):
    """``rdst_hip_select_limits``: (max_ranks, bits of the first digit, bits of the later digits, default cand_capacity, most
    levels one round can take) of :func:`select_device_tensor` for keys of ``dtype``; ``index_bytes``: 0 = keys only, 4 or 8."""
    _kind, nbytes, _levels = key_info(dtype)
    out = (ctypes.c_uint32 * 5)()
    _lib.check(_lib.load().rdst_hip_select_limits(nbytes, int(index_bytes), out))
    return tuple(int(v) for v in out)


def select_scratch_bytes(n, n_ranks, dtype, index_bytes=0, cand_capacity=0):
    """``rdst_hip_select_scratch_bytes``: bytes of scratch :func:`select_device_tensor` needs for ``n`` keys of ``dtype`` (0 for
    widths the entry is not built for).  Never ``n``-sized, and the same for every ``n_ranks``."""
    _kind, nbytes, _levels = key_info(dtype)
    return int(_lib.load().rdst_hip_select_scratch_bytes(int(n), int(n_ranks), nbytes, int(index_bytes), int(cand_capacity)))


def select_state(scratch):
    """``rdst_hip_debug_select_state`` (test hook, blocking): what the most recent round of :func:`select_device_tensor` on
    ``scratch`` decided — dict with ``levels``, ``groups`` (distinct prefixes at the end), ``candidates`` (collected) and
    ``exhausted`` (the digits ran out: the answers are the prefixes)."""
    import torch
    out = (ctypes.c_uint64 * 4)()
    with torch.cuda.device(scratch.device):
        _lib.check(_lib.load().rdst_hip_debug_select_state(_ptr(scratch), _stream_handle(scratch), out))
    return {"levels": int(out[0]), "groups": int(out[1]), "candidates": int(out[2]), "exhausted": int(out[3])}


def quantile_ranks(n, qs, method="lower"):
    """The ranks (0-based positions of the sorted array of ``n`` elements) that ``numpy.quantile(a, qs, method=...)`` indexes
    for ``method`` "lower", "higher" or "nearest", as a list of ints for :func:`select_device_tensor`.  Pure, host only."""
    import numpy as np
    n = int(n)
    if n < 1:
        raise ValueError("quantile_ranks needs n >= 1")
    q = np.atleast_1d(np.asarray(qs, dtype=np.float64))
    if q.size and not (np.all(q >= 0) and np.all(q <= 1)):
        raise ValueError("quantiles must lie in [0, 1]")
    virtual = (n - 1) * q                                   # numpy's virtual index for these three methods
    if method == "lower":
        r = np.floor(virtual)
    elif method == "higher":
        r = np.ceil(virtual)
    elif method == "nearest":
        r = np.around(virtual)                              # half to even, as numpy does
    else:
        raise ValueError('method must be "lower", "higher" or "nearest"')
    return [int(v) for v in np.clip(r, 0, n - 1).astype(np.int64)]


def select_device_tensor(keys, ranks, largest=False, index=None, scratch=None, cand_capacity=0, check=True, key=None):
    """``rdst_hip_select_device``: the keys of the 1-D contiguous HIP tensor ``keys`` (``key="u128"/"i128"``: shape (n, 2)) that
    stand at the positions ``ranks`` of the sort's order — ``largest``: of the descending order —, slot ``i`` for ``ranks[i]``,
    as a new tensor; ``keys`` is not modified and not sorted.  ``ranks``: a HOST sequence of ints below ``n``, any order,
    repeats allowed (:func:`quantile_ranks` makes one from quantiles); a device tensor is refused, never copied behind the
    caller's back.  ``index``: ``None`` for keys only, ``torch.int32`` or ``torch.int64`` to get the input position of each
    element of a stable argsort as well (4- and 8-byte keys).  ``scratch``: optional uint8 HIP tensor of at least
    :func:`select_scratch_bytes` bytes (allocated when omitted); ``cand_capacity``: 0 = the library's default, any value >= 1
    gives the same result.  Returns ``(out_keys, out_index or None)``.  The call only enqueues work on the tensor's current
    stream; ``check=False`` makes no blocking call at all (kernel failures then surface in :func:`device_status`)."""
    import torch
    kind, nbytes, levels, n, _per_key = _keys_operand("select_device_tensor", keys, key)
    if isinstance(ranks, torch.Tensor) and ranks.is_cuda:
        raise ValueError("select_device_tensor takes its ranks from the host: pass a list or ranks.tolist(), not a device tensor")
    ranks = [int(r) for r in (ranks.tolist() if hasattr(ranks, "tolist") else ranks)]
    if any(not 0 <= r < n for r in ranks):
        raise ValueError("every rank must lie in 0..len-1")
    index_bytes = _index_bytes(index)
    nr = len(ranks)
    out_keys = torch.empty((nr, 2) if _wide(key) else (nr,), dtype=keys.dtype, device=keys.device)
    out_index = None if index is None else torch.empty(nr, dtype=index, device=keys.device)
    if nr == 0:
        return out_keys, out_index
    need = int(_lib.load().rdst_hip_select_scratch_bytes(n, nr, nbytes, index_bytes, int(cand_capacity)))
    scratch, sbytes = _scratch(scratch, need, keys.device)
    _call(keys, check, "rdst_hip_select_device", _ptr(keys), n, (ctypes.c_uint64 * nr)(*ranks), nr, _ptr(out_keys), _ptr(out_index), index_bytes,
          _ptr(scratch), sbytes, int(cand_capacity), nbytes, kind, levels, _lib.RDST_TOPK_LARGEST if largest else 0)
    return out_keys, out_index


def segments_limits(dtype, val_bytes=0):
    """``rdst_hip_sort_segments_limits``: (wave_max, block_max) of the segmented sort for keys of ``dtype`` (a numpy / torch
    dtype or its name, ``"u128"`` / ``"i128"``) and values of ``val_bytes`` bytes (0: keys only) — the longest segment one
    wave takes and the longest one workgroup takes; longer ones go the whole-slice route and need ``tmp``."""
    _kind, nbytes, _levels = key_info(dtype)
    out = (ctypes.c_uint32 * 2)()
    _lib.check(_lib.load().rdst_hip_sort_segments_limits(nbytes, int(val_bytes), out))
    return int(out[0]), int(out[1])


def _host_offsets(offsets):
    """the segment borders as a contiguous uint64 numpy array on the host"""
    if _is_torch_tensor(offsets):
        offsets = offsets.detach().cpu().numpy()   # a device tensor: ONE copy to the host (the plan is made there)
    a = np.asarray(offsets)
    if a.ndim != 1 or a.size == 0:
        raise ValueError("offsets: a 1-D sequence of n_segments + 1 element indices")
    if a.dtype.kind not in "iu" or (a.dtype.kind == "i" and a.size and int(a.min()) < 0):
        raise ValueError("offsets must be non-negative integers")
    return np.ascontiguousarray(a, dtype=np.uint64)


def segments_plan(offsets, n, dtype, val_bytes=0):
    """``rdst_segments_plan`` (host only): the work list of a segmented sort over ``n`` elements — ``(items, counts,
    tmp_elems)`` with ``items`` a list of (start, len, segment) in the order the entry runs them, ``counts`` the numbers
    of wave-, block- and long-class items and ``tmp_elems`` the longest long segment (0: no ``tmp`` needed)."""
    off = _host_offsets(offsets)
    _kind, nbytes, _levels = key_info(dtype)
    lib = _lib.load()
    items = (_lib.SegmentItemC * max(1, off.size - 1))()
    counts = (ctypes.c_uint64 * 3)()
    tmp_elems = ctypes.c_uint64(0)
    _lib.check(lib.rdst_segments_plan(off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), off.size - 1, int(n), nbytes, int(val_bytes),
                                      items, off.size - 1, counts, ctypes.byref(tmp_elems)))
    total = int(counts[0] + counts[1] + counts[2])
    return [(int(it.start), int(it.len), int(it.seg)) for it in items[:total]], tuple(int(c) for c in counts), int(tmp_elems.value)


def _segments_operands(name, keys, values, key):
    """the keys and values of a segmented tensor wrapper, checked: (kind, nbytes, levels, n, per_key, vbytes)"""
    kind, nbytes, levels, n, per_key = _keys_operand(name, keys, key)
    if values is None:
        return kind, nbytes, levels, n, per_key, 0
    if values.device != keys.device or values.dim() != 1 or values.numel() != n or not values.is_contiguous():
        raise ValueError("values must be a contiguous 1-D tensor of the keys' length on the keys' device")
    return kind, nbytes, levels, n, per_key, values.element_size()


def sort_segments_device_tensor(keys, offsets, tmp=None, values=None, tmp_values=None, check=True, key=None):
    """``rdst_hip_sort_segments_device`` (with ``values``: ``rdst_hip_sort_segments_pairs_device``): sort every segment
    ``keys[offsets[s]:offsets[s + 1]]`` of a contiguous 1-D HIP tensor on its own, in one call (``key="u128"/"i128"``: shape
    (n, 2), offsets count keys).  ``offsets``: a sequence, a numpy array or a torch tensor of n_segments + 1 non-decreasing
    element indices; the library reads it on the HOST, so a device tensor is copied to the host once, here.  Elements
    outside [offsets[0], offsets[-1]) stay as they are.  ``values`` (4- or 8-byte elements, same length as ``keys``) are
    permuted with their keys; equal keys keep their input order.  ``tmp`` (and ``tmp_values``) are needed only when a segment
    is longer than ``segments_limits(...)[1]``: at least as many elements as the longest such segment; they are allocated
    when omitted and needed, and not at all otherwise.  Runs on the tensor's current stream; with ``check`` the call
    blocks and raises if a kernel reported failure.  Offsets that are computed on the device and should stay there:
    :func:`sort_segments_device_offsets_tensor`."""
    import torch
    kind, nbytes, levels, n, per_key, vbytes = _segments_operands("sort_segments_device_tensor", keys, values, key)
    off = _host_offsets(offsets)
    n_segments = off.size - 1
    lib = _lib.load()
    offp = off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    counts = (ctypes.c_uint64 * 3)()
    need = ctypes.c_uint64(0)
    rc = lib.rdst_segments_plan(offp, n_segments, n, nbytes, vbytes, None, 0, counts, ctypes.byref(need))
    if rc != _lib.RDST_OK and counts[0] + counts[1] + counts[2] == 0:   # (a list that does not fit capacity 0 is the expected answer)
        _lib.check(rc)
    need = int(need.value)
    tmp_elems = 0
    if need:
        if tmp is None:
            tmp = torch.empty(need * per_key, dtype=keys.dtype, device=keys.device)
        elif _mismatch(tmp, keys) or tmp.numel() < need * per_key:
            raise ValueError(f"tmp must be a contiguous tensor of the keys' dtype and device with at least {need} keys")
        tmp_elems = tmp.numel() // per_key
        if values is not None:
            if tmp_values is None:
                tmp_values = torch.empty(need, dtype=values.dtype, device=values.device)
            elif _mismatch(tmp_values, values) or tmp_values.numel() < need:
                raise ValueError(f"tmp_values must be a contiguous tensor of the values' dtype and device with at least {need} elements")
            tmp_elems = min(tmp_elems, tmp_values.numel())
    elif tmp is not None:
        tmp_elems = tmp.numel() // per_key
    if values is None:
        _call(keys, check, "rdst_hip_sort_segments_device", _ptr(keys), _ptr(tmp), tmp_elems, n, offp, n_segments, nbytes, kind, levels)
    else:
        _call(keys, check, "rdst_hip_sort_segments_pairs_device", _ptr(keys), _ptr(values), _ptr(tmp), _ptr(tmp_values), tmp_elems, n, offp,
              n_segments, nbytes, kind, levels, vbytes)


def topk_segments_limits(dtype, index_bytes=0):
    """``rdst_hip_topk_segments_limits``: (wave_max, block_max, stream_max, k_stream_max) of the segmented partial sort for
    keys of ``dtype`` (a dtype or its name, ``"u128"`` / ``"i128"``); ``index_bytes``: 0 = keys only, 4 or 8.  Segments up to
    wave_max take one wave, up to block_max one workgroup, up to stream_max — for k up to k_stream_max — one workgroup that
    streams them; everything else takes :func:`topk_device_tensor`'s route, one segment after another."""
    _kind, nbytes, _levels = key_info(dtype)
    out = (ctypes.c_uint32 * 4)()
    _lib.check(_lib.load().rdst_hip_topk_segments_limits(nbytes, int(index_bytes), out))
    return tuple(int(v) for v in out)


def topk_segments_scratch_bytes(n_segments, longest_segment, k, dtype, index_bytes=0):
    """``rdst_hip_topk_segments_scratch_bytes``: bytes of scratch :func:`topk_segments_device_tensor` needs for
    ``n_segments`` segments, the longest of ``longest_segment`` keys of ``dtype`` (0 for widths the entry is not built for)."""
    _kind, nbytes, _levels = key_info(dtype)
    return int(_lib.load().rdst_hip_topk_segments_scratch_bytes(int(n_segments), int(longest_segment), int(k), nbytes, int(index_bytes)))


def topk_segments_plan(offsets, n, k, dtype, index_bytes=0):
    """``rdst_topk_segments_plan`` (host only): the work list of a segmented partial sort over ``n`` elements — ``(items,
    counts, longest_far)`` with ``items`` a list of (start, len, segment) in the order the entry runs them, ``counts`` the
    numbers of wave-, block-, stream- and far-class items and ``longest_far`` the longest far segment (0: none)."""
    off = _host_offsets(offsets)
    _kind, nbytes, _levels = key_info(dtype)
    items = (_lib.SegmentItemC * max(1, off.size - 1))()
    counts = (ctypes.c_uint64 * 4)()
    longest = ctypes.c_uint64(0)
    _lib.check(_lib.load().rdst_topk_segments_plan(off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), off.size - 1, int(n), int(k), nbytes,
                                                   int(index_bytes), items, off.size - 1, counts, ctypes.byref(longest)))
    total = int(sum(counts))
    return [(int(it.start), int(it.len), int(it.seg)) for it in items[:total]], tuple(int(c) for c in counts), int(longest.value)


def set_topk_segments_stream_max(stream_max=0):
    """``rdst_hip_set_topk_segments_stream_max`` (test hook): the longest segment the stream class takes; 0 = the default."""
    _lib.check(_lib.load().rdst_hip_set_topk_segments_stream_max(int(stream_max)))


def _topk_rows_out(keys, key, per_key, index, n_segments, k, out):
    """(out_keys, out_index) of a segmented partial sort: the caller's pair, checked, or fresh (n_segments, k) tensors"""
    import torch
    if out is None:
        out_keys = torch.empty((n_segments, k, 2) if _wide(key) else (n_segments, k), dtype=keys.dtype, device=keys.device)
        return out_keys, None if index is None else torch.empty((n_segments, k), dtype=index, device=keys.device)
    out_keys, out_index = out
    if _mismatch(out_keys, keys) or out_keys.numel() != n_segments * k * per_key:
        raise ValueError("out keys: a contiguous tensor of the keys' dtype and device with n_segments * k keys")
    if (out_index is None) != (index is None) or (out_index is not None and (
            out_index.dtype != index or out_index.device != keys.device or not out_index.is_contiguous() or out_index.numel() != n_segments * k)):
        raise ValueError("out index: a contiguous tensor of dtype `index` on the keys' device with n_segments * k elements")
    return out_keys, out_index


def topk_segments_device_tensor(keys, offsets, k, largest=False, index=None, scratch=None, check=True, key=None, out=None):
    """``rdst_hip_topk_segments_device``: :func:`topk_device_tensor` for every segment ``keys[offsets[s]:offsets[s + 1]]`` of
    a contiguous 1-D HIP tensor, in one call (``key="u128"/"i128"``: shape (n, 2), offsets count keys).  ``offsets``: a
    sequence, a numpy array or a torch tensor of n_segments + 1 non-decreasing element indices, read on the HOST (a device
    tensor is copied to the host once, here).  Returns ``(out_keys, out_index or None)`` of shape (n_segments, k): row ``s``
    holds, in its first ``min(k, n_s)`` slots, the keys of segment ``s`` that come first in the sort's order — ``largest``:
    last, in descending order — and, with ``index`` (``torch.int32`` / ``torch.int64``; 4- and 8-byte keys), their positions
    inside the segment, equal keys in ascending position.  The slots from ``min(k, n_s)`` on are NOT written: pass ``out=
    (out_keys, out_index)`` to choose what they hold.  ``keys`` is not modified.  ``scratch``: optional uint8 HIP tensor of
    at least :func:`topk_segments_scratch_bytes` bytes, 256-byte aligned (allocated when omitted).  The call only enqueues
    work on the tensor's current stream; ``check=False`` makes no blocking call at all."""
    import torch
    kind, nbytes, levels, n, per_key = _keys_operand("topk_segments_device_tensor", keys, key)
    index_bytes = _index_bytes(index)
    k = int(k)
    if k < 0:
        raise ValueError("k must not be negative")
    off = _host_offsets(offsets)
    n_segments = off.size - 1
    out_keys, out_index = _topk_rows_out(keys, key, per_key, index, n_segments, k, out)
    if k == 0 or n_segments == 0:
        return out_keys, out_index
    longest = int((off[1:] - off[:-1]).max()) if bool((off[1:] >= off[:-1]).all()) else 0   # (a decreasing table: the library says so)
    need = int(_lib.load().rdst_hip_topk_segments_scratch_bytes(n_segments, longest, k, nbytes, index_bytes))
    scratch, sbytes = _scratch(scratch, need, keys.device)
    _call(keys, check, "rdst_hip_topk_segments_device", _ptr(keys), n, off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n_segments, k,
          _ptr(out_keys), _ptr(out_index), index_bytes, _ptr(scratch), sbytes, nbytes, kind, levels, _lib.RDST_TOPK_LARGEST if largest else 0)
    return out_keys, out_index


def topk_rows_tensor(keys2d, k, largest=False, index=None, scratch=None, check=True, out=None):
    """:func:`topk_segments_device_tensor` for the rows of a contiguous 2-D HIP tensor (a score or logits matrix): the ``k``
    first (``largest``: last) keys of every row and, with ``index``, their columns.  ``k`` may exceed the row length: the
    slots past it are not written."""
    _on_device("topk_rows_tensor", keys2d)
    if keys2d.dim() != 2 or not keys2d.is_contiguous():
        raise ValueError("topk_rows_tensor needs a contiguous 2-D tensor")
    rows, cols = int(keys2d.shape[0]), int(keys2d.shape[1])
    offsets = np.arange(rows + 1, dtype=np.uint64) * np.uint64(cols)
    return topk_segments_device_tensor(keys2d.reshape(-1), offsets, k, largest=largest, index=index, scratch=scratch, check=check, out=out)


def select_segments_limits(dtype, index_bytes=0):
    """``rdst_hip_select_segments_limits``: (wave_max, block_max, stream_max, max_ranks) of the segmented select for keys of
    ``dtype`` (a dtype or its name, ``"u128"`` / ``"i128"``); ``index_bytes``: 0 = keys only, 4 or 8.  Segments up to wave_max
    take one wave, up to block_max one workgroup, up to stream_max one workgroup that streams them; longer ones take
    :func:`select_device_tensor`'s route, one segment after another.  max_ranks: the rank specs of one round."""
    _kind, nbytes, _levels = key_info(dtype)
    out = (ctypes.c_uint32 * 4)()
    _lib.check(_lib.load().rdst_hip_select_segments_limits(nbytes, int(index_bytes), out))
    return tuple(int(v) for v in out)


def select_segments_scratch_bytes(n_segments, longest_segment, n_ranks, dtype, index_bytes=0):
    """``rdst_hip_select_segments_scratch_bytes``: bytes of scratch :func:`select_segments_device_tensor` needs for
    ``n_segments`` segments, the longest of ``longest_segment`` keys of ``dtype`` (0 for widths the entry is not built for)."""
    _kind, nbytes, _levels = key_info(dtype)
    return int(_lib.load().rdst_hip_select_segments_scratch_bytes(int(n_segments), int(longest_segment), int(n_ranks), nbytes, int(index_bytes)))


_RANK_MODES = {"lower": _lib.RDST_RANK_LOWER, "higher": _lib.RDST_RANK_HIGHER, "nearest": _lib.RDST_RANK_NEAREST}


def _rank_specs(ranks, quantiles, method):
    """the (num, den, mode) of every spec of a segmented select, the absolute ranks first, then the quantiles"""
    from fractions import Fraction
    if method not in _RANK_MODES:
        raise ValueError('method must be "lower", "higher" or "nearest"')
    specs = []
    for name, operand in (("ranks", ranks), ("quantiles", quantiles)):
        if _is_torch_tensor(operand) and operand.is_cuda:
            raise ValueError(f"select_segments_device_tensor takes its {name} from the host: pass a list, not a device tensor")
    for r in ([] if ranks is None else (ranks.tolist() if hasattr(ranks, "tolist") else ranks)):
        r = int(r)
        if not 0 <= r < 1 << 32:
            raise ValueError("an absolute rank lies in 0..2^32-1")
        specs.append((r, 0, 0))
    for q in ([] if quantiles is None else (quantiles.tolist() if hasattr(quantiles, "tolist") else quantiles)):
        if isinstance(q, Fraction):
            f = q
        elif isinstance(q, (tuple, list)):
            num, den = (int(v) for v in q)
            if den <= 0:
                raise ValueError("a quantile (num, den) has den > 0")
            if not 0 <= num <= den:
                raise ValueError("quantiles must lie in [0, 1]")
            if den >= 1 << 32:
                raise ValueError("a quantile's denominator must be below 2^32")
            specs.append((num, den, _RANK_MODES[method]))                  # as given: not reduced
            continue
        else:
            f = Fraction(repr(float(q)))                                    # the shortest decimal that names this float: 0.1 is 1/10
        if not 0 <= f <= 1:
            raise ValueError("quantiles must lie in [0, 1]")
        if f.denominator >= 1 << 32:
            raise ValueError("a quantile's denominator must be below 2^32")
        specs.append((f.numerator, f.denominator, _RANK_MODES[method]))
    return specs


def rank_for_length(n, rank=None, quantile=None, method="lower"):
    """``rdst_rank_for_length``: the rank that one spec — the absolute ``rank``, or the ``quantile`` (a ``Fraction``, a
    ``(num, den)`` pair or a float, taken at its shortest decimal form) rounded by ``method`` — stands for in a segment of
    ``n`` keys, or ``None`` where the segment has no such element.  Pure, host only, integer arithmetic."""
    if (rank is None) == (quantile is None):
        raise ValueError("rank_for_length takes a rank or a quantile")
    (num, den, mode), = _rank_specs(None if rank is None else [rank], None if quantile is None else [quantile], method)
    spec = _lib.RankSpecC(num, den, mode, 0)
    out = ctypes.c_uint64(0)
    rc = _lib.load().rdst_rank_for_length(ctypes.byref(spec), int(n), ctypes.byref(out))
    if rc < 0:
        _lib.check(rc)
    return int(out.value) if rc == 1 else None


def select_segments_device_tensor(keys, offsets, ranks=None, quantiles=None, method="lower", largest=False, index=None, scratch=None, check=True,
                                  key=None, out=None):
    """``rdst_hip_select_segments_device``: :func:`select_device_tensor` for every segment ``keys[offsets[s]:offsets[s + 1]]``
    of a contiguous 1-D HIP tensor, in one call (``key="u128"/"i128"``: shape (n, 2), offsets count keys).  Every segment
    resolves the specs against its own length ``n_s``: ``ranks`` holds ints, absolute ranks (a segment of ``n_s <= rank`` keys
    has no such element); ``quantiles`` holds ``fractions.Fraction``, ``(num, den)`` pairs or floats — a float is taken at its
    shortest decimal form, so 0.1 means 1/10 — and stands for the element ``numpy.quantile(..., method=method)`` indexes, with
    ``method`` "lower", "higher" or "nearest", in exact integer arithmetic (:func:`rank_for_length`).  Both lists may be given:
    the ranks come first, then the quantiles.  ``offsets``, ``ranks`` and ``quantiles`` are read on the HOST; device tensors
    are refused, never copied behind the caller's back.  Returns ``(out_keys, out_index or None)`` of shape (n_segments,
    n_ranks): slot ``i`` of row ``s`` holds the key of segment ``s`` at the rank of spec ``i`` in the sort's order —
    ``largest``: the descending order — and, with ``index`` (``torch.int32`` / ``torch.int64``; 4- and 8-byte keys), its
    position inside the segment as a stable argsort gives it.  Slots without a rank (empty segments, absolute ranks at or past
    the length) are NOT written: pass a pre-filled ``out=(out_keys, out_index)`` to recognise them.  ``keys`` is not
    modified.  ``scratch``: optional uint8 HIP tensor of at least :func:`select_segments_scratch_bytes` bytes, 256-byte aligned
    (allocated when omitted).  The call only enqueues work on the tensor's current stream; ``check=False`` makes no blocking
    call at all."""
    kind, nbytes, levels, n, per_key = _keys_operand("select_segments_device_tensor", keys, key)
    index_bytes = _index_bytes(index)
    if _is_torch_tensor(offsets) and offsets.is_cuda:
        raise ValueError("select_segments_device_tensor takes its offsets from the host: pass a list or offsets.tolist(), not a device tensor")
    specs = _rank_specs(ranks, quantiles, method)
    nr = len(specs)
    off = _host_offsets(offsets)
    n_segments = off.size - 1
    out_keys, out_index = _topk_rows_out(keys, key, per_key, index, n_segments, nr, out)
    if nr == 0 or n_segments == 0:
        return out_keys, out_index
    longest = int((off[1:] - off[:-1]).max()) if bool((off[1:] >= off[:-1]).all()) else 0   # (a decreasing table: the library says so)
    need = int(_lib.load().rdst_hip_select_segments_scratch_bytes(n_segments, longest, nr, nbytes, index_bytes))
    scratch, sbytes = _scratch(scratch, need, keys.device)
    table = (_lib.RankSpecC * nr)(*(_lib.RankSpecC(num, den, mode, 0) for num, den, mode in specs))
    _call(keys, check, "rdst_hip_select_segments_device", _ptr(keys), n, off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n_segments, table, nr,
          _ptr(out_keys), _ptr(out_index), index_bytes, _ptr(scratch), sbytes, nbytes, kind, levels, _lib.RDST_TOPK_LARGEST if largest else 0)
    return out_keys, out_index


def select_rows_tensor(keys2d, ranks=None, quantiles=None, method="lower", largest=False, index=None, scratch=None, check=True, out=None):
    """:func:`select_segments_device_tensor` for the rows of a contiguous 2-D HIP tensor: the median, the deciles, the k-th
    value of every row and, with ``index``, their columns."""
    _on_device("select_rows_tensor", keys2d)
    if keys2d.dim() != 2 or not keys2d.is_contiguous():
        raise ValueError("select_rows_tensor needs a contiguous 2-D tensor")
    rows, cols = int(keys2d.shape[0]), int(keys2d.shape[1])
    offsets = np.arange(rows + 1, dtype=np.uint64) * np.uint64(cols)
    return select_segments_device_tensor(keys2d.reshape(-1), offsets, ranks=ranks, quantiles=quantiles, method=method, largest=largest, index=index,
                                         scratch=scratch, check=check, out=out)


def segments_device_offsets_scratch_bytes(n_segments):
    """``rdst_hip_sort_segments_device_offsets_scratch_bytes``: bytes of scratch the device-offsets segmented sort needs for
    ``n_segments`` segments (0 for none, or for more than 2^30)."""
    return int(_lib.load().rdst_hip_sort_segments_device_offsets_scratch_bytes(int(n_segments)))


def _device_offsets(offsets, keys, n, unsigned_too=False):
    """(n_segments, offset_bytes) of a device-resident table of borders, checked without looking at its values;
    ``unsigned_too``: uint32 and uint64 tensors are taken as well"""
    import torch
    if not _is_torch_tensor(offsets) or not offsets.is_cuda or offsets.device != keys.device:
        raise ValueError("offsets must be a tensor on the keys' HIP device")
    if offsets.dim() != 1 or offsets.numel() == 0 or not offsets.is_contiguous():
        raise ValueError("offsets: a contiguous 1-D tensor of n_segments + 1 element indices")
    if unsigned_too and offsets.dtype in (getattr(torch, "uint32", None), getattr(torch, "uint64", None)):
        return offsets.numel() - 1, offsets.element_size()
    if offsets.dtype not in (torch.int32, torch.int64):
        raise ValueError("offsets must be int32 or int64 (read as unsigned: a negative value fails the device's check)")
    if offsets.dtype == torch.int32 and n >= 2**31:
        raise ValueError("int32 offsets need fewer than 2^31 keys")
    return offsets.numel() - 1, offsets.element_size()


def segments_plan_device(offsets, n, dtype, val_bytes=0, scratch=None):
    """``rdst_hip_debug_segments_plan_device`` (test hook, blocking): the work list the DEVICE plan makes of a device-resident
    ``offsets`` tensor (int32 / int64) over ``n`` elements — ``(items, counts, tmp_elems, flags)``, the first three as
    :func:`segments_plan` returns them; ``flags``: 1 = offsets decrease somewhere, 2 = the last offset lies past ``n`` (the
    other three then mean nothing)."""
    _kind, nbytes, _levels = key_info(dtype)
    n_segments, obytes = _device_offsets(offsets, offsets, 0)
    items = (_lib.SegmentItemC * max(1, n_segments))()
    counts = (ctypes.c_uint64 * 3)()
    tmp_elems = ctypes.c_uint64(0)
    flags = ctypes.c_uint32(0)
    scratch, sbytes = _scratch(scratch, segments_device_offsets_scratch_bytes(n_segments), offsets.device)
    _call(offsets, False, "rdst_hip_debug_segments_plan_device", _ptr(offsets), obytes, n_segments, int(n), nbytes, int(val_bytes), _ptr(scratch),
          sbytes, items, n_segments, counts, ctypes.byref(tmp_elems), ctypes.byref(flags))
    total = int(counts[0] + counts[1] + counts[2]) if not flags.value else 0
    return ([(int(it.start), int(it.len), int(it.seg)) for it in items[:total]], tuple(int(c) for c in counts), int(tmp_elems.value),
            int(flags.value))


def topk_segments_device_offsets_scratch_bytes(n_segments, far_capacity, k, dtype, index_bytes=0):
    """``rdst_hip_topk_segments_device_offsets_scratch_bytes``: bytes of scratch :func:`topk_segments_device_offsets_tensor`
    needs for ``n_segments`` segments of keys of ``dtype``: the plan and, with ``far_capacity`` > 0, behind it the partial
    sort's scratch for a far segment of ``far_capacity`` keys (0 for no segment, more than 2^30 of them, a ``far_capacity`` of
    2^32 or more, and widths the entry is not built for)."""
    _kind, nbytes, _levels = key_info(dtype)
    return int(_lib.load().rdst_hip_topk_segments_device_offsets_scratch_bytes(int(n_segments), int(far_capacity), int(k), nbytes, int(index_bytes)))


def topk_segments_plan_device(offsets, n, k, dtype, index_bytes=0, unbounded_stream=False, scratch=None):
    """``rdst_hip_debug_topk_segments_plan_device`` (test hook, blocking): the work list the DEVICE plan of
    :func:`topk_segments_device_offsets_tensor` makes of a device-resident ``offsets`` tensor (int32 / int64) over ``n``
    elements — ``(items, counts, longest_far, flags)``, the first three as :func:`topk_segments_plan` returns them;
    ``unbounded_stream``: the classes of the asynchronous mode, whose stream class has no upper length; ``flags``: 1 = offsets
    decrease somewhere, 2 = the last offset lies past ``n`` (the other three then mean nothing)."""
    _kind, nbytes, _levels = key_info(dtype)
    n_segments, obytes = _device_offsets(offsets, offsets, 0)
    items = (_lib.SegmentItemC * max(1, n_segments))()
    counts = (ctypes.c_uint64 * 4)()
    longest = ctypes.c_uint64(0)
    flags = ctypes.c_uint32(0)
    scratch, sbytes = _scratch(scratch, segments_device_offsets_scratch_bytes(n_segments), offsets.device)
    _call(offsets, False, "rdst_hip_debug_topk_segments_plan_device", _ptr(offsets), obytes, n_segments, int(n), int(k), nbytes, int(index_bytes),
          1 if unbounded_stream else 0, _ptr(scratch), sbytes, items, n_segments, counts, ctypes.byref(longest), ctypes.byref(flags))
    total = int(sum(counts)) if not flags.value else 0
    return ([(int(it.start), int(it.len), int(it.seg)) for it in items[:total]], tuple(int(c) for c in counts), int(longest.value),
            int(flags.value))


def topk_segments_device_offsets_tensor(keys, offsets, k, largest=False, index=None, scratch=None, far_capacity=0, check=True, key=None, out=None):
    """``rdst_hip_topk_segments_device_offsets``: :func:`topk_segments_device_tensor` for a table of borders that lives on the
    device — a CSR row pointer, a ``cumsum`` of lengths — and never visits the host.  ``offsets``: a contiguous 1-D int32 or
    int64 tensor on the keys' device with n_segments + 1 entries, read as unsigned and in stream order.  The result, ``index``
    and ``out`` are :func:`topk_segments_device_tensor`'s.  ``scratch``: optional uint8 tensor of at least
    :func:`topk_segments_device_offsets_scratch_bytes` bytes, 256-byte aligned (allocated when omitted).

    ``far_capacity=0`` is the fully asynchronous mode: nothing is copied to the host and nothing waited for (``check=False``
    makes no blocking call at all).  Every segment beyond ``topk_segments_limits(...)[1]`` keys is served by ONE workgroup,
    whatever its length — correct at any length, slow for very long rows — and ``k`` beyond ``topk_segments_limits(...)[3]``
    with such a segment, or a table that decreases or ends past the keys, writes nothing and raises from
    :func:`device_status` (here, with ``check``).  With ``far_capacity`` (the longest segment the call may meet; ``len(keys)``
    if nothing better is known) the classes are the host entry's; the call waits once for the stream to read the plan's
    counts, and an invalid table or a segment beyond ``far_capacity`` raises at once."""
    import torch
    kind, nbytes, levels, n, per_key = _keys_operand("topk_segments_device_offsets_tensor", keys, key)
    index_bytes = _index_bytes(index)
    k, far_capacity = int(k), int(far_capacity)
    if k < 0 or far_capacity < 0:
        raise ValueError("k and far_capacity must not be negative")
    n_segments, obytes = _device_offsets(offsets, keys, n)
    out_keys, out_index = _topk_rows_out(keys, key, per_key, index, n_segments, k, out)
    if k == 0 or n_segments == 0:
        return out_keys, out_index
    need = int(_lib.load().rdst_hip_topk_segments_device_offsets_scratch_bytes(n_segments, far_capacity, k, nbytes, index_bytes))
    scratch, sbytes = _scratch(scratch, need, keys.device)
    _call(keys, check, "rdst_hip_topk_segments_device_offsets", _ptr(keys), n, _ptr(offsets), obytes, n_segments, k, _ptr(out_keys), _ptr(out_index),
          index_bytes, _ptr(scratch), sbytes, far_capacity, nbytes, kind, levels, _lib.RDST_TOPK_LARGEST if largest else 0)
    return out_keys, out_index


def select_segments_device_offsets_scratch_bytes(n_segments, far_capacity, n_ranks, dtype, index_bytes=0):
    """``rdst_hip_select_segments_device_offsets_scratch_bytes``: bytes of scratch :func:`select_segments_device_offsets_tensor`
    needs for ``n_segments`` segments of keys of ``dtype``: the plan and, with ``far_capacity`` > 0, behind it the select's
    scratch for a far segment of ``far_capacity`` keys (0 for no segment, more than 2^30 of them, a ``far_capacity`` of 2^32 or
    more, and widths the entry is not built for)."""
    _kind, nbytes, _levels = key_info(dtype)
    return int(_lib.load().rdst_hip_select_segments_device_offsets_scratch_bytes(int(n_segments), int(far_capacity), int(n_ranks), nbytes,
                                                                                  int(index_bytes)))


def select_segments_device_offsets_tensor(keys, offsets, ranks=None, quantiles=None, method="lower", largest=False, index=None, scratch=None,
                                          far_capacity=0, check=True, key=None, out=None):
    """``rdst_hip_select_segments_device_offsets``: :func:`select_segments_device_tensor` for a table of borders that lives on
    the device — a CSR row pointer, a ``cumsum`` of lengths — and never visits the host.  ``offsets``: a contiguous 1-D int32,
    int64, uint32 or uint64 tensor on the keys' device with n_segments + 1 entries, read as unsigned and in stream order.
    ``ranks``, ``quantiles``, ``method``, the result, ``index`` and ``out`` are :func:`select_segments_device_tensor`'s; the
    specs stay on the host.  ``scratch``: optional uint8 tensor of at least
    :func:`select_segments_device_offsets_scratch_bytes` bytes, 256-byte aligned (allocated when omitted).

    ``far_capacity=0`` is the fully asynchronous mode: nothing is copied to the host and nothing waited for (``check=False``
    makes no blocking call at all).  Every segment beyond ``select_segments_limits(...)[1]`` keys is served by ONE workgroup,
    whatever its length — correct at any length, slow for very long rows, and slower still with ranks far apart — and only a
    table that decreases or ends past the keys can fail: it writes nothing and raises from :func:`device_status` (here, with
    ``check``).  With ``far_capacity`` (the longest segment the call may meet; ``len(keys)`` if nothing better is known) the
    classes are the host entry's; the call waits once for the stream to read the plan's counts, and an invalid table or a
    segment beyond ``far_capacity`` raises at once."""
    kind, nbytes, levels, n, per_key = _keys_operand("select_segments_device_offsets_tensor", keys, key)
    index_bytes = _index_bytes(index)
    far_capacity = int(far_capacity)
    if far_capacity < 0:
        raise ValueError("far_capacity must not be negative")
    specs = _rank_specs(ranks, quantiles, method)
    nr = len(specs)
    n_segments, obytes = _device_offsets(offsets, keys, n, unsigned_too=True)
    out_keys, out_index = _topk_rows_out(keys, key, per_key, index, n_segments, nr, out)
    if nr == 0 or n_segments == 0:
        return out_keys, out_index
    need = int(_lib.load().rdst_hip_select_segments_device_offsets_scratch_bytes(n_segments, far_capacity, nr, nbytes, index_bytes))
    scratch, sbytes = _scratch(scratch, need, keys.device)
    table = (_lib.RankSpecC * nr)(*(_lib.RankSpecC(num, den, mode, 0) for num, den, mode in specs))
    _call(keys, check, "rdst_hip_select_segments_device_offsets", _ptr(keys), n, _ptr(offsets), obytes, n_segments, table, nr, _ptr(out_keys),
          _ptr(out_index), index_bytes, _ptr(scratch), sbytes, far_capacity, nbytes, kind, levels, _lib.RDST_TOPK_LARGEST if largest else 0)
    return out_keys, out_index


def runs_limits(dtype):
    """``rdst_hip_runs_limits``: (keys per tile, status words per look-back round trip) of :func:`runs_device_tensor` for keys
    of ``dtype`` (a numpy / torch dtype or its name, ``"u128"`` / ``"i128"``)."""
    _kind, nbytes, _levels = key_info(dtype)
    out = (ctypes.c_uint32 * 2)()
    _lib.check(_lib.load().rdst_hip_runs_limits(nbytes, out))
    return int(out[0]), int(out[1])


def runs_scratch_bytes(n, dtype):
    """``rdst_hip_runs_scratch_bytes``: bytes of scratch :func:`runs_device_tensor` needs for ``n`` keys of ``dtype`` (0 for
    2^32 keys and more)."""
    _kind, nbytes, _levels = key_info(dtype)
    return int(_lib.load().rdst_hip_runs_scratch_bytes(int(n), nbytes))


def runs_device_tensor(keys, length=None, capacity=None, starts="int64", pad=False, scratch=None, check=True, key=None, out=None):
    """``rdst_hip_runs_device``: the runs of bit-identical keys of the 1-D contiguous HIP tensor ``keys`` (``key="u128"/"i128"``:
    shape (n, 2)) — ``Vec::dedup`` / ``unique_consecutive`` on the device; on sorted keys, the distinct keys and where each
    one's group begins.  Returns ``(run_keys, starts, n_runs)``: the key of every run (``capacity`` entries; the capacity
    defaults to ``len(keys)``), the position of its first element (``capacity + 1`` entries of dtype ``starts``:
    ``torch.int64``, ``torch.int32`` or their names; ``None`` skips the table) and the number of
    runs R as a one-element device tensor that this function never reads.  ``starts[:R + 1]`` is a CSR table of the groups
    (``starts[R]`` = the length) that every ``*_device_offsets_tensor`` wrapper takes; with ``pad`` the slots behind R hold
    the length too, so ``starts`` as a whole is a table of ``capacity`` segments whose surplus ones are empty — nobody has to
    read R.  Slots behind R are otherwise left as they were.  ``length``: an optional one-element device tensor (see
    :func:`sort_device_devlen_tensor`): only the first ``m`` keys are looked at.  More runs than ``capacity`` (> 0) keeps the
    first ``capacity`` complete, stores the true R and raises from :func:`device_status` (bit 64); ``capacity=0`` only
    counts.  ``out``: optional ``(run_keys, starts, n_runs)`` tensors to write into; a ``None`` in place of
    the first or the second skips that output (the call is then keys-only, starts-only or, with both, a count), one in place
    of the third is allocated.
    ``scratch``: optional uint8 tensor of at least :func:`runs_scratch_bytes` bytes, 256-byte aligned.  ``keys`` is not
    modified.  The call only enqueues work on the tensor's current stream; ``check=False`` makes no blocking call at all."""
    import torch
    kind, nbytes, levels, n, per_key = _keys_operand("runs_device_tensor", keys, key)
    devlen = _device_length(_WHOLE if length is None else length, keys) or (None, 0)
    capacity = n if capacity is None else int(capacity)
    if capacity < 0:
        raise ValueError("capacity must not be negative")
    if starts is not None:
        starts = getattr(torch, starts) if isinstance(starts, str) else starts
        if starts not in (torch.int32, torch.int64):
            raise ValueError("starts must be None, torch.int32 or torch.int64")
    o_keys, o_starts, o_count = out if out is not None else (None, None, None)
    if out is not None and o_starts is None:                                    # either way of skipping the table
        starts = None
    if starts is None:
        o_starts = None
    if pad and starts is None:
        raise ValueError("pad fills the starts: it needs them")
    if starts is not None:
        off_dtype = starts
    else:                                                                       # no table: the caller's n_runs decides, else int64
        off_dtype = o_count.dtype if o_count is not None and o_count.dtype in (torch.int32, torch.int64) else torch.int64
    if out is None:
        o_keys = torch.empty((capacity, 2) if _wide(key) else (capacity,), dtype=keys.dtype, device=keys.device)
    if starts is not None and o_starts is None:
        o_starts = torch.empty(capacity + 1, dtype=off_dtype, device=keys.device)
    if o_count is None:
        o_count = torch.empty(1, dtype=off_dtype, device=keys.device)
    for t, dtype, need, what in ((o_keys, keys.dtype, capacity * per_key, "run_keys"), (o_starts, off_dtype, capacity + 1, "starts"), (o_count, off_dtype, 1, "n_runs")):
        if t is not None and (t.dtype != dtype or t.device != keys.device or not t.is_contiguous() or t.numel() < need):
            raise ValueError(f"out: {what} must be a contiguous {dtype} tensor on the keys' device with at least {need} elements")
    need = int(_lib.load().rdst_hip_runs_scratch_bytes(n, nbytes))
    scratch, sbytes = _scratch(scratch, need, keys.device)
    _call(keys, check, "rdst_hip_runs_device", _ptr(keys, empty_is_null=True), n, *devlen, _ptr(o_keys), _ptr(o_starts), _ptr(o_count), o_count.element_size(),
          capacity, _ptr(scratch), sbytes, nbytes, kind, levels, _lib.RDST_RUNS_PAD_STARTS if pad else 0)
    return o_keys, o_starts, o_count


def search_limits(dtype):
    """``rdst_hip_search_limits``: (needles per workgroup tile, splitters, keys a workgroup stages in LDS) of
    :func:`search_device_tensor` for keys of ``dtype`` (a numpy / torch dtype or its name, ``"u128"`` / ``"i128"``)."""
    _kind, nbytes, _levels = key_info(dtype)
    out = (ctypes.c_uint32 * 3)()
    _lib.check(_lib.load().rdst_hip_search_limits(nbytes, out))
    return int(out[0]), int(out[1]), int(out[2])


def search_scratch_bytes(n, n_needles, dtype):
    """``rdst_hip_search_scratch_bytes``: bytes of scratch :func:`search_device_tensor` needs for ``n_needles`` needles in ``n``
    keys of ``dtype`` (0 for 2^32 and more of either)."""
    _kind, nbytes, _levels = key_info(dtype)
    return int(_lib.load().rdst_hip_search_scratch_bytes(int(n), int(n_needles), nbytes))


def search_state(scratch):
    """``rdst_hip_debug_search_state`` (test hook, blocking): what the most recent :func:`search_device_tensor` on ``scratch``
    did — dict with ``m`` (the haystack's length as the device read it), ``staged`` and ``table`` (tiles of needles per path)
    and ``past`` (1: m was past the capacity)."""
    import torch
    out = (ctypes.c_uint64 * 4)()
    with torch.cuda.device(scratch.device):
        _lib.check(_lib.load().rdst_hip_debug_search_state(_ptr(scratch), _stream_handle(scratch), out))
    return {"m": int(out[0]), "staged": int(out[1]), "table": int(out[2]), "past": int(out[3])}


def search_device_tensor(sorted_keys, needles, side="left", length=None, positions="int64", scratch=None, check=True, key=None, out=None):
    """``rdst_hip_search_device``: where each of ``needles`` falls in the sorted 1-D contiguous HIP tensor ``sorted_keys``
    (``key="u128"/"i128"``: both of shape (n, 2)) — ``numpy.searchsorted`` / ``partition_point`` in THE SORT'S order: the
    mapped bits, so -0.0 comes before +0.0, every NaN has its place and 16-byte keys are keys.  ``side="left"``: the number of
    keys strictly before each needle; ``"right"``: before or equal; ``"both"``: the tuple ``(lower, upper)``, whose
    difference is the needle's multiplicity.  The result has one entry per needle, of dtype ``positions`` (``torch.int64``,
    ``torch.int32`` or their names).  ``length``: an optional one-element device tensor (see
    :func:`sort_device_devlen_tensor`): only the first ``m`` keys are the haystack — the R that :func:`runs_device_tensor`
    has just written, never read by the host; ``m`` past ``len(sorted_keys)`` writes nothing and raises from
    :func:`device_status` (bit 32).  ``out``: the tensor (for ``"both"``: the two tensors) to write into.  ``scratch``:
    optional uint8 tensor of at least :func:`search_scratch_bytes` bytes, 256-byte aligned.  Neither input is modified, and
    they may be the same tensor.  An unsorted haystack gives positions in [0, m] that mean nothing.  The call only enqueues
    work on the tensor's current stream; ``check=False`` makes no blocking call at all."""
    import torch
    kind, nbytes, levels, n, _per_key = _keys_operand("search_device_tensor", sorted_keys, key)
    _kind, _nbytes, _levels, n_needles, _per = _keys_operand("search_device_tensor", needles, key)
    if needles.dtype != sorted_keys.dtype or needles.device != sorted_keys.device:
        raise ValueError("needles must have the dtype and the device of sorted_keys")
    if side not in ("left", "right", "both"):
        raise ValueError('side must be "left", "right" or "both"')
    devlen = _device_length(_WHOLE if length is None else length, sorted_keys) or (None, 0)
    positions = getattr(torch, positions) if isinstance(positions, str) else positions
    if positions not in (torch.int32, torch.int64):
        raise ValueError("positions must be torch.int32 or torch.int64")
    given = (None, None) if out is None else (tuple(out) if side == "both" else (out, None) if side == "left" else (None, out))
    if len(given) != 2 or (side == "both" and out is not None and (given[0] is None or given[1] is None)):
        raise ValueError('out: one tensor, or (lower, upper) for side="both"')
    want = (side != "right", side != "left")
    outs = []
    for t, wanted, what in zip(given, want, ("lower", "upper")):
        if not wanted:
            t = None
        elif t is None:
            t = torch.empty(n_needles, dtype=positions, device=sorted_keys.device)
        elif t.dtype != positions or t.device != sorted_keys.device or not t.is_contiguous() or t.numel() < n_needles:
            raise ValueError(f"out: {what} must be a contiguous {positions} tensor on the keys' device with at least {n_needles} elements")
        outs.append(t)
    need = int(_lib.load().rdst_hip_search_scratch_bytes(n, n_needles, nbytes))
    scratch, sbytes = _scratch(scratch, need, sorted_keys.device)
    _call(sorted_keys, check, "rdst_hip_search_device", _ptr(sorted_keys, empty_is_null=True), n, *devlen, _ptr(needles, empty_is_null=True), n_needles,
          _ptr(outs[0]), _ptr(outs[1]), outs[0].element_size() if outs[0] is not None else outs[1].element_size(), _ptr(scratch), sbytes, nbytes, kind, levels, 0)
    return tuple(outs) if side == "both" else outs[0] if side == "left" else outs[1]


def unique_device_tensor(keys, counts=False, scratch=None, check=True, key=None, inverse=False):
    """Sort, then dedup, on the device: a clone of ``keys``, :func:`sort_device_tensor` on it, then
    :func:`runs_device_tensor`.  Returns ``(unique_keys, n_unique)`` — ``len(keys)`` slots of which the first R hold the distinct
    keys in the sort's order, and R as a one-element device tensor —, with ``counts`` ``(unique_keys, counts, n_unique)``:
    the multiplicity of every distinct key, 0 in the slots behind R (``starts[1:] - starts[:-1]`` of the padded table, a torch
    expression).  With ``inverse`` the tuple gets one more element at its end: an int64 tensor with
    ``unique_keys[inverse[i]] == keys[i]`` bit for bit (:func:`search_device_tensor` of the distinct keys for ``keys``, with
    ``length=n_unique``).  ``keys`` is not modified.  Nothing is copied to the host; ``check=False`` makes no blocking call."""
    work = keys.clone()
    sort_device_tensor(work, check=False, key=key)
    uniq, starts, count = runs_device_tensor(work, starts="int64" if counts else None, pad=counts, scratch=scratch, check=check and not inverse, key=key)
    result = (uniq, starts[1:] - starts[:-1], count) if counts else (uniq, count)
    if not inverse:
        return result
    return result + (search_device_tensor(uniq, keys, length=count, check=check, key=key),)


def sort_segments_device_offsets_tensor(keys, offsets, tmp=None, values=None, tmp_values=None, scratch=None, check=True, key=None):
    """``rdst_hip_sort_segments_device_offsets`` (with ``values``: ``rdst_hip_sort_segments_pairs_device_offsets``):
    :func:`sort_segments_device_tensor` for a table of borders that lives on the device — a CSR row pointer, a ``cumsum`` of
    lengths — and never visits the host.  ``offsets``: a contiguous 1-D int32 or int64 tensor on the keys' device with
    n_segments + 1 entries, read as unsigned and in stream order (int32 only below 2^31 keys).  ``scratch``: optional uint8
    tensor of at least ``segments_device_offsets_scratch_bytes(n_segments)`` bytes, 256-byte aligned (allocated when
    omitted); calls on one stream may share it.

    ``tmp=None`` is the fully asynchronous mode: nothing is copied to the host and nothing waited for; a table that
    decreases or ends past the keys, or a segment longer than ``segments_limits(...)[1]``, leaves every key and value as
    it was and raises from :func:`device_status` (here, with ``check``).  With ``tmp`` (and ``tmp_values`` for pairs; as
    many elements as the longest segment may have) longer segments are sorted too; the call then waits once for the
    stream to read the plan's counts, and an invalid table or a ``tmp`` that is too short raises at once."""
    import torch
    kind, nbytes, levels, n, per_key, vbytes = _segments_operands("sort_segments_device_offsets_tensor", keys, values, key)
    n_segments, obytes = _device_offsets(offsets, keys, n)
    tmp_elems = 0
    if tmp is not None:
        if _mismatch(tmp, keys):
            raise ValueError("tmp must be a contiguous tensor of the keys' dtype and device")
        tmp_elems = tmp.numel() // per_key
        if values is not None:
            if tmp_values is None:
                tmp_values = torch.empty(tmp_elems, dtype=values.dtype, device=values.device)
            elif _mismatch(tmp_values, values):
                raise ValueError("tmp_values must be a contiguous tensor of the values' dtype and device")
            tmp_elems = min(tmp_elems, tmp_values.numel())
    elif tmp_values is not None:
        raise ValueError("tmp_values without tmp")
    scratch, sbytes = _scratch(scratch, segments_device_offsets_scratch_bytes(n_segments), keys.device)
    if not tmp_elems:
        tmp = tmp_values = None
    if values is None:
        _call(keys, check, "rdst_hip_sort_segments_device_offsets", _ptr(keys), _ptr(tmp), tmp_elems, n, _ptr(offsets), obytes, n_segments,
              nbytes, kind, levels, _ptr(scratch), sbytes)
    else:
        _call(keys, check, "rdst_hip_sort_segments_pairs_device_offsets", _ptr(keys), _ptr(values), _ptr(tmp), _ptr(tmp_values), tmp_elems, n,
              _ptr(offsets), obytes, n_segments, nbytes, kind, levels, vbytes, _ptr(scratch), sbytes)


def segments_nowait_scratch_bytes(n_segments, n, dtype, val_bytes=0):
    """``rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes``: bytes of scratch the nowait segmented sort needs for
    ``n_segments`` segments of an array of ``n`` keys of ``dtype`` (a dtype or a key name, as for :func:`segments_limits`)
    with ``val_bytes``-byte values (0: keys only).  0 for no segment, more than 2^30 segments, 2^32 keys or more, and widths
    the sort does not take."""
    _kind, nbytes, _levels = key_info(dtype)
    return int(_lib.load().rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes(int(n_segments), int(n), nbytes, int(val_bytes)))


def sort_segments_device_offsets_nowait_tensor(keys, offsets, tmp=None, values=None, tmp_values=None, scratch=None, check=True, key=None):
    """``rdst_hip_sort_segments_device_offsets_nowait`` (with ``values``: ``rdst_hip_sort_segments_pairs_device_offsets_nowait``):
    :func:`sort_segments_device_offsets_tensor` without a visit to the host for segments of ANY length.  Segments beyond
    ``segments_limits(...)[1]`` are sorted on the device too, tile by tile between the keys and ``tmp``; nothing is copied to
    the host and nothing waited for.  ``tmp`` (and ``tmp_values`` for pairs): as many elements as the keys, allocated on the
    keys' device when omitted; only the positions of long segments are written.  ``scratch``: optional uint8 tensor of at
    least ``segments_nowait_scratch_bytes(n_segments, n, dtype, val_bytes)`` bytes, 256-byte aligned (allocated when
    omitted); calls on one stream may share it.  A table that decreases or ends past the keys leaves every key, value and
    tmp element as it was and raises from :func:`device_status` (here, with ``check``)."""
    import torch
    kind, nbytes, levels, n, _per_key, vbytes = _segments_operands("sort_segments_device_offsets_nowait_tensor", keys, values, key)
    if n >= 2**32:
        raise ValueError("the nowait segmented sort takes fewer than 2^32 keys")
    if values is None and tmp_values is not None:
        raise ValueError("tmp_values without values")
    n_segments, obytes = _device_offsets(offsets, keys, n)
    if tmp is None:
        tmp = torch.empty_like(keys)
    elif _mismatch(tmp, keys) or tmp.numel() < keys.numel():
        raise ValueError("tmp must be a contiguous tensor of the keys' dtype and device with at least as many elements")
    if values is not None:
        if tmp_values is None:
            tmp_values = torch.empty_like(values)
        elif _mismatch(tmp_values, values) or tmp_values.numel() < n:
            raise ValueError("tmp_values must be a contiguous tensor of the values' dtype and device with at least as many elements")
    need = int(_lib.load().rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes(n_segments, n, nbytes, vbytes))
    scratch, sbytes = _scratch(scratch, need, keys.device)

    def ptr(t):
        return _ptr(t, empty_is_null=True)

    if values is None:
        _call(keys, check, "rdst_hip_sort_segments_device_offsets_nowait", ptr(keys), ptr(tmp), n, ptr(offsets), obytes, n_segments, nbytes, kind,
              levels, ptr(scratch), sbytes)
    else:
        _call(keys, check, "rdst_hip_sort_segments_pairs_device_offsets_nowait", ptr(keys), ptr(values), ptr(tmp), ptr(tmp_values), n, ptr(offsets),
              obytes, n_segments, nbytes, kind, levels, vbytes, ptr(scratch), sbytes)


def sort_records_by_key(records, key_field):
    """Device route for a slice of structs whose ``RadixKey`` is one built-in field
    (benches/struct_sort.rs:11-27, examples/impl_radix_key.rs:32-56): ``records`` is a 2-D
    HIP tensor (n, fields), ``key_field`` the column holding the key (the tensor's dtype decides the key kind).  Extracts (key, row index), sorts the pairs on
    the device, gathers the rows; returns the reordered tensor (rows with equal keys keep their order)."""
    import torch
    if records.dim() != 2 or not records.is_cuda:
        raise ValueError("records must be a 2-D HIP tensor (n, fields)")
    n = records.shape[0]
    if n <= 1:
        return records.clone()
    keys = records[:, key_field].contiguous()
    idx = torch.arange(n, dtype=torch.int32 if n < 2**31 else torch.int64, device=records.device)
    sort_pairs_device_tensor(keys, idx)
    return records.index_select(0, idx.long() if idx.dtype != torch.int64 else idx)


def sort_device_tensor_lowmem(keys, scratch=None):
    """``rdst_hip_sort_device_lowmem``: sort a 1-D contiguous HIP tensor IN PLACE with a scratch of only ``scratch.numel()``
    elements (default: len / 64, at least 65 536) instead of a second array — the device twin of the route
    ``with_low_mem_tuner()`` selects in the reference (Regions / Ska: src/tuners/low_memory_tuner.rs:36-41,
    src/sorts/regions_sort.rs:51-286).  Blocking.  Same result as :func:`sort_device_tensor`."""
    import torch
    if not keys.is_cuda or keys.dim() != 1 or not keys.is_contiguous():
        raise ValueError("sort_device_tensor_lowmem needs a contiguous 1-D tensor on a HIP device")
    kind, nbytes, levels = key_info(keys.dtype)
    n = keys.numel()
    if n <= 1:
        return
    if scratch is None:
        scratch = torch.empty(max(65536, -(-n // 64)), dtype=keys.dtype, device=keys.device)
    elif scratch.dtype != keys.dtype or scratch.device != keys.device or not scratch.is_contiguous():
        raise ValueError("scratch must be a contiguous tensor of the same dtype and device")
    _call(keys, False, "rdst_hip_sort_device_lowmem", _ptr(keys), n, nbytes, kind, levels, _ptr(scratch), scratch.numel())


def partition_device(keys, level, digit, scratch=None):
    """``rdst_hip_partition_device`` — ``partition_index`` (src/sort_utils.rs:295-331) with the predicate "digit `level` of
    the key == `digit`": those keys first, the others after, in place; returns the split index.  Blocking."""
    import torch
    if not keys.is_cuda or keys.dim() != 1 or not keys.is_contiguous():
        raise ValueError("partition_device needs a contiguous 1-D tensor on a HIP device")
    kind, nbytes, _levels = key_info(keys.dtype)
    n = keys.numel()
    if scratch is None:
        scratch = torch.empty(max(65536, -(-n // 64)), dtype=keys.dtype, device=keys.device)
    split = ctypes.c_uint64(0)
    _call(keys, False, "rdst_hip_partition_device", _ptr(keys), n, nbytes, kind, int(level), int(digit), _ptr(scratch), scratch.numel(),
          ctypes.byref(split))
    return int(split.value)


def _ask_current_stream(device, entry, *out):
    """`entry(stream, *out)` for the current stream of `device` (None: the current device)"""
    import torch
    with torch.cuda.device(device):
        _lib.check(getattr(_lib.load(), entry)(_current_stream(), *out))


def device_status(device=None):
    """Block on the current stream and raise if a kernel reported failure."""
    _ask_current_stream(device, "rdst_hip_device_status")


def _host_call(entry, arr, n, device, *args):
    """the tail of a host-slice wrapper: `entry(arr's memory, n, *args, opts)` (H2D, device sort, D2H; blocking)"""
    opts = _lib.HipOptsC(int(device), 0, 0)
    _lib.check(getattr(_lib.load(), entry)(ctypes.c_void_p(arr.ctypes.data), n, *args, ctypes.byref(opts)))


def sort_host_array(arr, device=-1, key=None):
    """``rdst_hip_sort`` on a host numpy array (H2D, device sort, D2H), in place.  ``key="bytes"``: a uint8
    array of shape (n, N), N in 1..RDST_BYTES_MAX_N (4096), each row one ``[u8; N]`` key (src/radix_key_impl.rs:78-85:
    rows end up in lexicographic order)."""
    if not isinstance(arr, np.ndarray) or not arr.flags.c_contiguous or not arr.flags.writeable:
        raise ValueError("need a writeable C-contiguous 1-D numpy array (rdst sorts a mutable slice)")
    if key == "bytes":
        _check_bytes_rows(arr.shape, arr.dtype == np.uint8)
        kind, nbytes, levels = _lib.RDST_KEY_BYTES_BE, int(arr.shape[1]), int(arr.shape[1])
    else:
        if _wide(key):
            _check_wide_shape(arr.shape, arr.dtype.itemsize)
        elif arr.ndim != 1:
            raise ValueError("need a writeable C-contiguous 1-D numpy array (rdst sorts a mutable slice)")
        kind, nbytes, levels = key_info(key if key else arr.dtype.name)
    if arr.nbytes // nbytes <= 1:
        return
    _host_call("rdst_hip_sort", arr, arr.nbytes // nbytes, device, nbytes, kind, levels)


class KeyField:
    """One field of a described key (``rdst_key_field``, include/rdst_hip.h): ``bytes`` bytes at ``offset`` inside the
    record, mapped as ``kind`` (``"unsigned"``, ``"signed"``, ``"float"``, ``"bytes"`` or an ``RDST_KEY_*`` integer);
    ``descending`` complements the mapped bytes.  A sequence of them, most significant first, is the ``RadixKey`` with
    ``LEVELS`` = the sum of the widths (examples/impl_radix_key.rs:32-56)."""
    KINDS = {"unsigned": _lib.RDST_KEY_UNSIGNED, "signed": _lib.RDST_KEY_SIGNED, "float": _lib.RDST_KEY_FLOAT,
             "bytes": _lib.RDST_KEY_BYTES_BE}
    __slots__ = ("offset", "bytes", "kind", "descending")

    def __init__(self, offset, bytes, kind, descending=False):  # noqa: A002  (the C field's name)
        self.offset, self.bytes = int(offset), int(bytes)
        self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        self.descending = bool(descending)

    def __repr__(self):
        return f"KeyField({self.offset}, {self.bytes}, {self.kind}, descending={self.descending})"

    def __eq__(self, other):
        return isinstance(other, KeyField) and self.as_tuple() == other.as_tuple()

    def __hash__(self):
        return hash(self.as_tuple())

    def as_tuple(self):
        """(offset, bytes, kind, flags) as the C struct holds them"""
        return self.offset, self.bytes, self.kind, _lib.RDST_FIELD_DESCENDING if self.descending else 0


def _field_table(fields):
    fields = list(fields)
    if not all(isinstance(f, KeyField) for f in fields):
        raise TypeError("a key description is a sequence of KeyField")
    return (_lib.KeyFieldC * max(1, len(fields)))(*[_lib.KeyFieldC(*f.as_tuple()) for f in fields]), len(fields)


def sort_records_device_tensor(records, fields, scratch=None, check=True):
    """``rdst_hip_sort_records_by_fields_device``: sort the rows of a contiguous (n, R) uint8 HIP tensor in place by the key
    ``fields`` describes (a sequence of :class:`KeyField`, most significant first); rows with equal keys keep their order.
    The row base needs no alignment.  ``scratch``: optional uint8 HIP tensor of at least
    ``rdst_hip_sort_records_by_fields_scratch_bytes`` bytes, 256-byte aligned (allocated when omitted).  Runs on the
    tensor's current stream: keys of up to 8 bytes stay asynchronous unless ``check``, longer ones block (the tie counts
    come to the host)."""
    _sort_records_rows("sort_records_device_tensor", "rdst_hip_sort_records_by_fields_device", records, fields, scratch, check)


def sort_records_device_nowait_tensor(records, fields, scratch=None, check=True):
    """``rdst_hip_sort_records_by_fields_device_nowait``: :func:`sort_records_device_tensor` without the host in the loop,
    for keys of up to ``RDST_BYTES_NOWAIT_MAX_N`` (128) bytes; the same arguments, the same scratch size and, bit for bit,
    the same result.  The call only enqueues work on the tensor's current stream; ``check=False`` makes no blocking call
    at all (kernel failures then surface in :func:`device_status`)."""
    _sort_records_rows("sort_records_device_nowait_tensor", "rdst_hip_sort_records_by_fields_device_nowait", records, fields, scratch, check)


def _sort_records_rows(name, entry, records, fields, scratch, check):
    import torch
    _on_device(name, records)
    if records.dim() != 2 or records.dtype != torch.uint8 or not records.is_contiguous():
        raise ValueError("records must be a contiguous (n, R) uint8 tensor, one row per record")
    n, rec_bytes = int(records.shape[0]), int(records.shape[1])
    table, nf = _field_table(fields)
    need = int(_lib.load().rdst_hip_sort_records_by_fields_scratch_bytes(n, rec_bytes, table, nf))
    scratch, sbytes = _scratch(scratch, need, records.device, "records")
    # unlike the [u8; N] rows, zero or one record still reach the library: it is the library that checks the description
    # (and enqueues nothing then, so there is no status to wait for)
    _call(records, check and n > 1, entry, _ptr(records), n, rec_bytes, table, nf, _ptr(scratch), sbytes)


def _is_byte_string(ftype):
    return (ftype.subdtype is not None and ftype.subdtype[0] == np.uint8 and len(ftype.subdtype[1]) == 1) or \
        (ftype.kind in "SV" and ftype.fields is None and ftype.subdtype is None)


def _field_key(ftype):
    """(kind, bytes) of one field of a numpy structured dtype: a byte string or a built-in key type"""
    if _is_byte_string(ftype):
        return _lib.RDST_KEY_BYTES_BE, ftype.itemsize
    return key_info(ftype.name)[:2]


def key_fields_of(dtype, names):
    """The :class:`KeyField` table of a numpy structured dtype for the fields ``names``: each a field name or a
    ``(name, "desc")`` / ``(name, "asc")`` pair, most significant first.  Offsets, widths and kinds come from the dtype:
    integers and floats of any built-in width, and byte strings (``('u1', (N,))``, ``'S<N>'``, ``'V<N>'``)."""
    out = []
    for item in names:
        name, direction = (item, "asc") if isinstance(item, str) else item
        if direction not in ("asc", "desc"):
            raise ValueError(f"field direction is 'asc' or 'desc', not {direction!r}")
        ftype, offset = dtype.fields[name][:2]
        if ftype.byteorder == ">":   # (never a byte string's; sort_host_records' single-field form does not look)
            raise TypeError(f"field {name!r} is big-endian; built-in key fields are read little-endian")
        kind, nbytes = _field_key(ftype)
        out.append(KeyField(int(offset), nbytes, kind, direction == "desc"))
    return out


def sort_host_records(arr, field, device=-1):
    """``rdst_hip_sort_records`` on a numpy structured array, in place: the rows are ordered by ``field``
    (a 4- or 8-byte integer or float field, or a ``[u8; N]`` byte string: ``('u1', (N,))``, ``'S<N>'`` or ``'V<N>'``, N up to
    RDST_BYTES_MAX_N, lexicographic); rows with equal keys keep their order.  ``field`` may also be a sequence of field
    names or ``(name, "desc")`` pairs, most significant first (``rdst_hip_sort_records_by_fields``): any built-in width,
    any offset; or a sequence of :class:`KeyField`."""
    if not isinstance(arr, np.ndarray) or arr.dtype.fields is None or arr.ndim != 1:
        raise ValueError("need a 1-D numpy structured array")
    if not arr.flags.c_contiguous or not arr.flags.writeable:
        raise ValueError("need a writeable C-contiguous array (rdst sorts a mutable slice)")
    if not isinstance(field, str):
        field = list(field)
        fields = field if field and all(isinstance(f, KeyField) for f in field) else key_fields_of(arr.dtype, field)
        table, nf = _field_table(fields)
        _host_call("rdst_hip_sort_records_by_fields", arr, arr.shape[0], device, arr.dtype.itemsize, table, nf)
        return
    ftype, offset = arr.dtype.fields[field][:2]
    kind, nbytes = _field_key(ftype)
    if kind == _lib.RDST_KEY_BYTES_BE and not 1 <= nbytes <= _lib.RDST_BYTES_MAX_N:
        raise ValueError(f"[u8; N] key fields: N in 1..{_lib.RDST_BYTES_MAX_N}")
    if arr.shape[0] <= 1:
        return
    _host_call("rdst_hip_sort_records", arr, arr.shape[0], device, arr.dtype.itemsize, int(offset), nbytes, kind)


class RadixSortBuilder:
    """src/radix_sort_builder.rs:8-158.  ``with_parallel`` and the CPU tuners are accepted for
    source compatibility; they select among the reference's CPU algorithms, which this package
    does not ship, so on the device route they only take part in the top-level
    ``pick_algorithm`` call (a tuner that does not return a ``Gpu*`` algorithm raises)."""

    def __init__(self, data, key=None):
        self._data = data
        self._key = key
        self._multi_threaded = True
        self._tuner: Tuner = GpuTuner(0)

    def with_parallel(self, parallel: bool):
        self._multi_threaded = bool(parallel)
        return self

    def with_low_mem_tuner(self):
        self._tuner = LowMemoryTuner()
        return self

    def with_single_threaded_tuner(self):
        self._tuner = SingleThreadedTuner()
        return self

    def with_tuner(self, tuner: Tuner):
        if not hasattr(tuner, "pick_algorithm"):
            raise TypeError("tuner must implement pick_algorithm(p, counts)")
        self._tuner = tuner
        return self

    def _len_and_levels(self):
        d = self._data
        if self._key == "bytes":  # [u8; N] rows of a (n, N) uint8 array
            return int(d.shape[0]), int(d.shape[1])
        if self._key:
            _, nbytes, levels = key_info(self._key)
            total = d.numel() * d.element_size() if _is_torch_tensor(d) else d.nbytes
            return total // nbytes, levels
        if _is_torch_tensor(d):
            return d.numel(), key_info(d.dtype)[2]
        return d.size, key_info(d.dtype.name)[2]

    def sort(self):
        """Sorts in place and returns None, like the reference — except when the tuner answers
        ``Algorithm.GpuSharded``: the slice is then this rank's shard of a distributed array, the call is
        collective over the default torch.distributed group (one rank per GPU), and the return value is a NEW
        tensor, this rank's contiguous slice of the global order (its length differs from the input's, so it
        cannot be written in place)."""
        n, levels = self._len_and_levels()
        algo = None
        try:
            import torch.distributed as dist
            collective = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        except Exception:  # noqa: BLE001
            collective = False
        # radix_sort_builder.rs:151.  Only a custom tuner can answer GpuSharded (the stock ones and the default device
        # tuner never do): only then may an empty or one-key shard have to take part in a collective sort.
        custom = not isinstance(self._tuner, (GpuTuner, LowMemoryTuner, SingleThreadedTuner, StandardTuner))
        if n <= 1 and not (collective and custom):
            return
        if isinstance(self._tuner, LowMemoryTuner) and not self._key:
            # with_low_mem_tuner(): the reference trades speed for memory (Ska / Regions instead of the out-of-place
            # sorts, src/tuners/low_memory_tuner.rs:13-43); so does the device: in place, scratch of len / 64 elements
            import torch
            if _is_torch_tensor(self._data):
                sort_device_tensor_lowmem(self._data)
            else:
                dev = torch.from_numpy(self._data.view(_same_width_int(self._data.dtype))).cuda().view(getattr(torch, self._data.dtype.name))
                sort_device_tensor_lowmem(dev)
                self._data.view(_same_width_int(self._data.dtype))[:] = dev.view(getattr(torch, np.dtype(_same_width_int(self._data.dtype)).name)).cpu().numpy()
            return
        if not isinstance(self._tuner, GpuTuner):
            if self._key:
                raise NotImplementedError("custom tuners are wired for the dtype-described key types only")
            # top-level pick_algorithm, as Sorter::handle_chunk does (src/sorter.rs:67-76)
            counts = top_level_counts(self._data)
            algo = self._tuner.pick_algorithm(
                TuningParams(threads=1, level=levels - 1, total_levels=levels, input_len=n, parent_len=None), counts)
        if collective and custom and _is_torch_tensor(self._data):
            # GpuSharded is collective: every rank must take it or none (a rank that stays out leaves the others waiting in
            # the all-gather for ever).  One small all-reduce settles it; disagreement raises on EVERY rank.
            import torch
            import torch.distributed as dist
            dev = self._data.device if dist.get_backend() == "nccl" else "cpu"
            votes = torch.tensor([int(algo == Algorithm.GpuSharded), int(algo != Algorithm.GpuSharded)], dtype=torch.int32, device=dev)
            dist.all_reduce(votes)
            yes, no = (int(v) for v in votes.cpu())
            if yes and no:
                raise RuntimeError(f"the tuner answered Algorithm.GpuSharded on {yes} rank(s) and something else on {no}: a tuner that "
                                   "can route to the sharded sort must answer identically on all ranks (decide on world-level "
                                   "quantities, not on the local shard)")
        if algo is not None and algo not in (Algorithm.GpuLsd, Algorithm.GpuSharded):
            raise NotImplementedError(
                f"tuner picked {Algorithm(algo).name}: the CPU algorithms stay in the reference crate; "
                "this package implements the device routes (Algorithm.GpuLsd, Algorithm.GpuSharded) only")
        if algo == Algorithm.GpuSharded:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()):
                raise RuntimeError("Algorithm.GpuSharded is collective: it needs an initialised torch.distributed "
                                   "process group with one rank per GPU (rdst_amd/sharded.py)")
            if not _is_torch_tensor(self._data) or self._key:
                raise NotImplementedError("Algorithm.GpuSharded sorts a HIP tensor of a dtype-described key type (this rank's shard)")
            from .sharded import sharded_sort
            out = sharded_sort(self._data)
            if out.is_cuda:
                device_status(out.device)
            return out
        if _is_torch_tensor(self._data):
            if self._key == "bytes":
                sort_bytes_device_tensor(self._data)
                return
            sort_device_tensor(self._data, key=self._key)
        else:
            sort_host_array(self._data, key=self._key)


def top_level_counts(data):
    """256-bin histogram of the most significant level (what handle_chunk hands the tuner)."""
    import torch
    if _is_torch_tensor(data):
        dev = data
    else:
        dev = torch.from_numpy(data.view(_same_width_int(data.dtype))).cuda()
        dev = dev.view(getattr(torch, data.dtype.name))
    counts, _, _, _ = level_counts(dev, key_info(dev.dtype)[2] - 1)
    return counts


def _same_width_int(dt):
    return {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[np.dtype(dt).itemsize]


def level_counts(keys, level):
    """Parity hook: (counts[256], already_sorted, first_digit, last_digit) of one level
    (get_counts_with_ends, src/sort_utils.rs:109-180) over a HIP tensor."""
    kind, nbytes, _ = key_info(keys.dtype)
    counts = (ctypes.c_uint64 * 256)()
    srt, first, last = ctypes.c_uint8(1), ctypes.c_uint8(0), ctypes.c_uint8(0)
    _call(keys, False, "rdst_hip_level_counts", _ptr(keys), keys.numel(), nbytes, kind, level, counts, ctypes.byref(srt), ctypes.byref(first),
          ctypes.byref(last))
    return list(counts), bool(srt.value), first.value, last.value


def all_level_counts(keys):
    """Parity hook for the fused histogram kernel: numpy uint64 array [levels, 256]."""
    kind, nbytes, levels = key_info(keys.dtype)
    out = np.zeros((levels, 256), dtype=np.uint64)
    _call(keys, False, "rdst_hip_all_level_counts", _ptr(keys), keys.numel(), nbytes, kind, levels, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    return out


def scatter_level(src, level, dst=None):
    """Parity hook: one stable counting-sort pass on digit ``level`` (out_of_place_sort,
    src/sorts/out_of_place_sort.rs:52-108).  Returns (dst tensor, counts[256])."""
    import torch
    kind, nbytes, _ = key_info(src.dtype)
    if dst is None:
        dst = torch.empty_like(src)
    counts = np.zeros(256, dtype=np.uint64)
    _call(src, False, "rdst_hip_scatter_level", _ptr(src), _ptr(dst), src.numel(), nbytes, kind, level, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    return dst, counts


def radix_sort_builder(data, key=None) -> RadixSortBuilder:
    """``RadixSort::radix_sort_builder`` (src/radix_sort.rs:29-31 / :42-44).  ``key``: "u128" / "i128"
    for (n, 2) limb containers, "bytes" for a (n, N) uint8 array of ``[u8; N]`` keys; otherwise the key
    type is the container's dtype."""
    if key == "bytes":
        n_levels = int(data.shape[1]) if getattr(data, "ndim", 0) == 2 else 0
    else:
        n_levels = key_info(key if key else (data.dtype if _is_torch_tensor(data) else data.dtype.name))[2]
    assert n_levels != 0, "RadixKey must have at least 1 level"  # radix_sort_builder.rs:22
    return RadixSortBuilder(data, key)


def radix_sort_unstable(data, key=None) -> None:
    """``RadixSort::radix_sort_unstable`` (src/radix_sort.rs:25-27 / :38-40)."""
    radix_sort_builder(data, key).sort()


def set_tuning(pass_config=-1, hist_blocks_per_cu=0, chain_split=True, fast_rank=True, small_sort=True):
    _lib.check(_lib.load().rdst_hip_set_tuning(int(pass_config), int(hist_blocks_per_cu)))
    _lib.check(_lib.load().rdst_hip_set_chain_split(int(bool(chain_split))))
    _lib.check(_lib.load().rdst_hip_set_fast_rank(2 if fast_rank == 2 else int(bool(fast_rank))))
    _lib.check(_lib.load().rdst_hip_set_small_sort(int(bool(small_sort))))


def set_profiling(enabled: bool):
    """Record HIP events between the kernels of every following sort (rdst_hip_set_profiling)."""
    _lib.check(_lib.load().rdst_hip_set_profiling(int(bool(enabled))))


def profile_runs() -> int:
    """Number of pipelines recorded since profiling was enabled (current device)."""
    return int(_lib.load().rdst_hip_profile_runs())


STAGE_NAMES = {1: "clear", 2: "histogram", 3: "scan", 4: "pass", 5: "copy_back", 6: "histogram16", 7: "route", 8: "local_sort", 10: "msd_pass_a", 11: "msd_pass_b", 12: "sample", 13: "segments", 14: "segments_tiled", 15: "topk", 16: "select"}


def profile_run(run: int, levels: int):
    """Stage times (ms) of recorded run `run` (negative: from the most recent): dict with 'clear',
    'histogram', 'scan', 'passes' (one per level the call covered; a level the plan skipped shows its
    early-exit time), 'copy_back', and on calls that tried the hybrid route 'histogram16', 'route',
    'local_sort'; 'stages' lists (name, level or None, ms) in launch order."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    kinds = (ctypes.c_uint32 * 64)()
    n, nk = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _lib.check(lib.rdst_hip_profile_run(int(run), buf, 64, ctypes.byref(n)))
    _lib.check(lib.rdst_hip_profile_run_stages(int(run), kinds, 64, ctypes.byref(nk)))
    if n.value == 0 or n.value != nk.value:
        return None
    out = {"clear": 0.0, "histogram": 0.0, "scan": 0.0, "passes": [], "copy_back": 0.0, "stages": []}
    for i in range(n.value):
        code, level = kinds[i] & 0xFF, (kinds[i] >> 8) & 0xFF
        name = STAGE_NAMES.get(code, f"stage{code}")
        ms = float(buf[i])
        out["stages"].append((name, level if name in ("pass", "topk", "select") else None, ms))   # (topk: the select level; 255 = the collection pass)
        if name == "pass":
            out["passes"].append(ms)
        else:
            out[name] = out.get(name, 0.0) + ms
    if len(out["passes"]) < levels:
        return None
    return out


# rdst_hip_set_hybrid's modes by name (the integers include/rdst_hip.h documents; kRouteModes in csrc/rdst_kernels.hip)
ROUTE_MODES = {
    "lsd": 0,                # LSD only (False)
    "default": 1,            # 4- and 8-byte keys try the atomic route, then the hybrid one, then LSD (True)
    "ranked": 2,             # "k1h" with the generic ranked K4
    "count_whole_keys": 3,   # "k1h" with the counting K4 fed whole keys (no 16-bit hand-off)
    "no_presample": 5,       # "k1h" without the key sample
    "wide_one_block": 6,     # "k1h", 8-byte keys with the one-block-per-CU K4
    "k1h": 7,                # the K1h hybrid route for every width
    "atomic_4_only": 8,      # the atomic route for 4-byte keys only (8-byte keys on the hybrid route)
    "no_expand": 9,          # "k1h" without the expanding K4 (buckets up to one tile only)
    "atomic_then_lsd": 10,   # the default without the hybrid route as the atomic route's first fallback
    "no_giants": 11,         # the default without the giant kernels (a 4-byte bucket of 65 536 keys and more: LSD route)
    "no_exact_msd": 12,      # the default without the exact form of the MSD passes
    "no_predict": 14,        # the default without the sample's prediction of the LSD route
    "wide2": 15,             # the default with the second form of the 8-byte K4 (local_wide2_sort_kernel)
    "no_split": 16,          # the default without the split of slices beyond the atomic route's window (run_split_sort)
    "split_always": 17,      # the default with that split at every length, in eight parts (tests)
}


def set_hybrid(enabled=True, min_len=0):
    """Route choice knob (rdst_hip_set_hybrid): consider the byte-saving routes for sorts of at least `min_len` keys (0 = the
    built-in threshold).  `enabled`: True / False, or an A/B and test mode by its name or integer (ROUTE_MODES); anything else
    counts as its truth value."""
    if isinstance(enabled, str):
        enabled = ROUTE_MODES[enabled]
    _lib.check(_lib.load().rdst_hip_set_hybrid(int(enabled) if enabled in ROUTE_MODES.values() else int(bool(enabled)), int(min_len)))


def release_workspace(device=None) -> None:
    """Give the library-owned device workspace back (rdst_hip_release_workspace): the byte-saving routes keep 1.7 x the
    slice between calls.  Blocking; the next sort allocates again."""
    import torch
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        _lib.check(_lib.load().rdst_hip_release_workspace())


def last_route(device=None) -> str:
    """'lsd', 'hybrid' or 'atomic': the route the most recent sort on the current stream's device took."""
    r = ctypes.c_uint32(0)
    _ask_current_stream(device, "rdst_hip_last_route", ctypes.byref(r))
    return {1: "hybrid", 2: "atomic"}.get(r.value, "lsd")


SAMPLE_WORDS = ("win_shift", "win_top", "gross_skew", "top_skew", "low_dups", "predict_lsd")


def last_sample(device=None) -> dict:
    """What the key sample of the most recent sort on the current stream's device decided (rdst_hip_debug_last_sample, a test
    hook): the six plan words of SAMPLE_WORDS by name; all zero when the sort took no sample."""
    out = (ctypes.c_uint32 * 6)()
    _ask_current_stream(device, "rdst_hip_debug_last_sample", out)
    return {name: int(out[i]) for i, name in enumerate(SAMPLE_WORDS)}


def last_profile(levels: int):
    return profile_run(-1, levels) if profile_runs() else None
