"""The argument errors of the tensor wrappers that take no segments (rdst_amd.sort_device_tensor, sort_pairs_device_tensor,
their _devlen twins, topk_device_tensor, the [u8; N] and described-key wrappers, sort_device_tensor_lowmem, partition_device):
every operand a wrapper refuses raises an error that names what is wrong, before a sort is enqueued; where a wrapper returns
early (at most one key, k == 0, one row) the checks that come later are not made, and that order is asserted as well.  A
device is needed only because the wrappers insist on device tensors: device_status() stays clean and every operand keeps
its bits.  The segmented wrappers: test_gpu_segments_wrapper_args.py."""
import pytest

pytestmark = pytest.mark.gpu

SORT, DEVLEN, TOPK = "sort_device_tensor", "sort_device_devlen_tensor", "topk_device_tensor"
PAIRS, PAIRS_DEVLEN = "sort_pairs_device_tensor", "sort_pairs_device_devlen_tensor"
BYTES = ("sort_bytes_device_tensor", "sort_bytes_device_nowait_tensor")
RECORDS = ("sort_records_device_tensor", "sort_records_device_nowait_tensor")
LOWMEM, PARTITION = "sort_device_tensor_lowmem", "partition_device"

SLICE = "keys must be a contiguous 1-D tensor (rdst sorts a slice)"
TMP = "tmp must be a contiguous tensor of the same dtype/device with at least len elements"
TMP_PAIR = "tmp tensors must match their originals in dtype, device and length"
LENGTH = "length must be a contiguous one-element tensor of dtype int32, int64, uint32 or uint64"


def _keys(n=8, dtype=None, device="cuda"):
    import torch
    return torch.arange(n, 0, -1, dtype=dtype or torch.int32, device=device)


def _limbs(rows=4):
    import torch
    return torch.arange(2 * rows, dtype=torch.int64, device="cuda").view(torch.uint64).reshape(rows, 2)


def _length(value=8, dtype=None, device="cuda"):
    import torch
    return torch.tensor([value], dtype=dtype or torch.int64, device=device)


def _bits(t):
    import torch
    return t.contiguous().view(torch.uint8)


def _snapshot(args, kw):
    import torch
    tensors = [a for a in list(args) + list(kw.values()) if isinstance(a, torch.Tensor)]
    return [(t, _bits(t).clone()) for t in tensors]


def _unchanged(snapshot, name):
    import torch
    for t, before in snapshot:
        assert torch.equal(before, _bits(t)), name


def _with_defaults(name, kw):
    """the arguments a wrapper cannot do without, where a case does not set them itself"""
    if name in (DEVLEN, PAIRS_DEVLEN):
        kw.setdefault("length", _length())
    if name == TOPK:
        kw.setdefault("k", 3)
    if name == PARTITION:
        kw.setdefault("level", 0)
        kw.setdefault("digit", 1)
    return kw


def _refused(gpu, name, part, *args, exc=ValueError, **kw):
    kw = _with_defaults(name, kw)
    snapshot = _snapshot(args, kw)
    with pytest.raises(exc) as e:
        getattr(gpu, name)(*args, **kw)
    assert type(e.value) is exc and part in str(e.value), (name, repr(e.value))
    _unchanged(snapshot, name)


def _accepted(gpu, name, *args, **kw):
    """the call returns without a sort: nothing was checked after the point at which it returned"""
    kw = _with_defaults(name, kw)
    snapshot = _snapshot(args, kw)
    out = getattr(gpu, name)(*args, **kw)
    _unchanged(snapshot, name)
    return out


# ---- keys only: sort_device_tensor, sort_device_devlen_tensor, topk_device_tensor ----

@pytest.mark.parametrize("name", (SORT, DEVLEN, TOPK))
def test_keys(gpu, name):
    import torch
    _refused(gpu, name, f"{name} needs a tensor on a HIP device", _keys(device="cpu"))
    _refused(gpu, name, SLICE, _keys().reshape(4, 2))
    _refused(gpu, name, SLICE, _keys(16)[::2])
    _refused(gpu, name, "a 128-bit key container has shape (n, 2)", _keys(dtype=torch.int64), key="u128")
    _refused(gpu, name, SLICE, torch.zeros(4, 4, dtype=torch.int64, device="cuda").view(torch.uint64)[:, :2], key="u128")
    _refused(gpu, name, "no device RadixKey mapping", torch.zeros(8, dtype=torch.float16, device="cuda"), exc=TypeError)
    gpu.device_status()


@pytest.mark.parametrize("name", (SORT, DEVLEN))
def test_tmp(gpu, name):
    import torch
    _refused(gpu, name, TMP, _keys(), tmp=torch.zeros(8, dtype=torch.float32, device="cuda"))
    _refused(gpu, name, TMP, _keys(), tmp=torch.zeros(7, dtype=torch.int32, device="cuda"))
    _refused(gpu, name, TMP, _keys(), tmp=torch.zeros(16, dtype=torch.int32, device="cuda")[::2])
    _refused(gpu, name, TMP, _keys(), tmp=torch.zeros(8, dtype=torch.int32))
    _refused(gpu, name, TMP, _limbs(), tmp=torch.zeros(3, 2, dtype=torch.int64, device="cuda").view(torch.uint64), key="u128")
    # at most one key: the call returns before it looks at tmp
    for keys, key in ((_keys(1), None), (_keys(0), None), (_limbs(1), "u128")):
        for tmp in (torch.zeros(8, dtype=torch.float32, device="cuda"), torch.zeros(0, dtype=torch.int32)):
            assert _accepted(gpu, name, keys, tmp=tmp, key=key) is None
    gpu.device_status()


@pytest.mark.parametrize("name", (DEVLEN, PAIRS_DEVLEN))
def test_length(gpu, name):
    import torch

    def operands(n=8):
        return (_keys(n),) if name == DEVLEN else (_keys(n), torch.arange(n, dtype=torch.int32, device="cuda"))

    _refused(gpu, name, LENGTH, *operands(), length=torch.tensor([8.0], device="cuda"))
    _refused(gpu, name, LENGTH, *operands(), length=_length(dtype=torch.int16))
    _refused(gpu, name, LENGTH, *operands(), length=torch.tensor([8, 8], device="cuda"))
    # (a strided view has two elements at least: torch calls every one-element tensor contiguous)
    _refused(gpu, name, LENGTH, *operands(), length=torch.tensor([8, 0, 8, 0], device="cuda")[::2])
    _refused(gpu, name, LENGTH, *operands(), length=8)
    _refused(gpu, name, "length must live on the keys' device", *operands(), length=_length(device="cpu"))
    # the key type comes first, the length before the capacity <= 1 return, tmp after it
    bad_keys = (torch.zeros(8, dtype=torch.float16, device="cuda"),) + operands()[1:]
    _refused(gpu, name, "no device RadixKey mapping", *bad_keys, length=8, exc=TypeError)
    _refused(gpu, name, LENGTH, *operands(1), length=8)
    _refused(gpu, name, "length must live on the keys' device", *operands(0), length=_length(device="cpu"))
    bad_tmp = {"tmp" if name == DEVLEN else "tmp_keys": torch.zeros(8, dtype=torch.float32)}
    assert _accepted(gpu, name, *operands(1), length=_length(1, dtype=torch.int32), **bad_tmp) is None
    gpu.device_status()


# ---- keys and values: sort_pairs_device_tensor, sort_pairs_device_devlen_tensor ----

@pytest.mark.parametrize("name", (PAIRS, PAIRS_DEVLEN))
def test_pairs(gpu, name):
    import torch

    def values(n=8, device="cuda"):
        return torch.arange(n, dtype=torch.int32, device=device)

    part = "keys and values must live on the same HIP device"
    _refused(gpu, name, part, _keys(), values(device="cpu"))
    _refused(gpu, name, part, _keys(device="cpu"), values())
    _refused(gpu, name, part, _keys(device="cpu"), values(device="cpu"))
    part = "keys and values must be 1-D tensors of the same length"
    _refused(gpu, name, part, _keys(), values(7))
    _refused(gpu, name, part, _keys().reshape(4, 2), values())
    _refused(gpu, name, part, _keys(), values().reshape(4, 2))
    part = "keys and values must be contiguous"
    _refused(gpu, name, part, _keys(16)[::2], values())
    _refused(gpu, name, part, _keys(), values(16)[::2])
    _refused(gpu, name, "no device RadixKey mapping", torch.zeros(8, dtype=torch.float16, device="cuda"), values(), exc=TypeError)
    for which in ("tmp_keys", "tmp_values"):
        _refused(gpu, name, TMP_PAIR, _keys(), values(), **{which: torch.zeros(8, dtype=torch.float32, device="cuda")})
        _refused(gpu, name, TMP_PAIR, _keys(), values(), **{which: torch.zeros(7, dtype=torch.int32, device="cuda")})
        _refused(gpu, name, TMP_PAIR, _keys(), values(), **{which: torch.zeros(16, dtype=torch.int32, device="cuda")[::2]})
        _refused(gpu, name, TMP_PAIR, _keys(), values(), **{which: torch.zeros(8, dtype=torch.int32)})
        # at most one pair: the call returns before it looks at either tmp
        assert _accepted(gpu, name, _keys(1), values(1), **{which: torch.zeros(8, dtype=torch.float32)}) is None
        assert _accepted(gpu, name, _keys(0), values(0), **{which: torch.zeros(8, dtype=torch.float32)}) is None
    gpu.device_status()


# ---- topk_device_tensor ----

def test_topk_k_and_index(gpu):
    import torch
    _refused(gpu, TOPK, "k must lie in 0..len", _keys(), k=-1)
    _refused(gpu, TOPK, "k must lie in 0..len", _keys(), k=9)
    _refused(gpu, TOPK, "k must lie in 0..len", _limbs(), k=5, key="u128")        # four keys, not eight limbs
    _refused(gpu, TOPK, "index must be None, torch.int32 or torch.int64", _keys(), index=torch.int16)
    _refused(gpu, TOPK, "k must lie in 0..len", _keys(), k=-1, index=torch.int16)   # k first
    gpu.device_status()


def test_topk_nothing_asked(gpu):
    """k == 0: empty outputs of the right shape and dtype, and the scratch is not looked at"""
    import torch
    for scratch in (None, torch.empty(1, dtype=torch.uint8), torch.empty(16, dtype=torch.uint8, device="cuda")[::2]):
        out, idx = _accepted(gpu, TOPK, _keys(), k=0, scratch=scratch)
        assert tuple(out.shape) == (0,) and out.dtype == torch.int32 and out.is_cuda and idx is None
        out, idx = _accepted(gpu, TOPK, _keys(), k=0, index=torch.int64, scratch=scratch)
        assert tuple(out.shape) == (0,) and out.dtype == torch.int32
        assert tuple(idx.shape) == (0,) and idx.dtype == torch.int64 and idx.is_cuda
        out, idx = _accepted(gpu, TOPK, _limbs(), k=0, scratch=scratch, key="u128")
        assert tuple(out.shape) == (0, 2) and out.dtype == torch.uint64 and out.is_cuda and idx is None
    out, idx = _accepted(gpu, TOPK, _keys(0), k=0, index=torch.int32)
    assert tuple(out.shape) == (0,) and tuple(idx.shape) == (0,) and idx.dtype == torch.int32
    gpu.device_status()


def test_topk_scratch(gpu):
    import torch
    need = gpu.topk_scratch_bytes(8, 3, "int32")
    assert need > 0
    part = f"scratch must be a contiguous tensor on the keys' device with at least {need} bytes"
    _refused(gpu, TOPK, part, _keys(), scratch=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    _refused(gpu, TOPK, part, _keys(), scratch=torch.empty(need, dtype=torch.uint8))
    _refused(gpu, TOPK, part, _keys(), scratch=torch.empty(2 * need, dtype=torch.uint8, device="cuda")[::2])
    need = gpu.topk_scratch_bytes(8, 3, "int32", 4)
    part = f"scratch must be a contiguous tensor on the keys' device with at least {need} bytes"
    _refused(gpu, TOPK, part, _keys(), index=torch.int32, scratch=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    gpu.device_status()


# ---- [u8; N] rows and described keys ----

@pytest.mark.parametrize("name", BYTES)
def test_bytes_rows(gpu, name):
    import torch
    from rdst_amd import _lib

    def rows(n=4, width=4, dtype=torch.uint8, device="cuda"):
        return torch.zeros(n, width, dtype=dtype, device=device)

    _refused(gpu, name, f"{name} needs a tensor on a HIP device", rows(device="cpu"))
    part = "[u8; N] keys: a uint8 container of shape (n, N) with N in 1..4096"
    _refused(gpu, name, part, rows(dtype=torch.int8))
    _refused(gpu, name, part, torch.zeros(16, dtype=torch.uint8, device="cuda"))
    _refused(gpu, name, part, rows(width=0))
    _refused(gpu, name, part, rows(n=2, width=4097))
    _refused(gpu, name, "rows must be a contiguous (n, N) tensor", rows(width=8)[:, ::2])
    need = int(_lib.load().rdst_hip_sort_bytes_scratch_bytes(4, 4))
    assert need > 0
    part = f"scratch must be a contiguous tensor on the rows' device with at least {need} bytes"
    _refused(gpu, name, part, rows(), scratch=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    _refused(gpu, name, part, rows(), scratch=torch.empty(need, dtype=torch.uint8))
    _refused(gpu, name, part, rows(), scratch=torch.empty(2 * need, dtype=torch.uint8, device="cuda")[::2])
    # at most one row: the call returns before it looks at the scratch
    assert _accepted(gpu, name, rows(n=1), scratch=torch.empty(1, dtype=torch.uint8)) is None
    assert _accepted(gpu, name, rows(n=0), scratch=torch.empty(16, dtype=torch.uint8, device="cuda")[::2]) is None
    gpu.device_status()


@pytest.mark.parametrize("name", RECORDS)
def test_records(gpu, name):
    import torch
    from rdst_amd import _lib
    from rdst_amd.radix_sort import _field_table
    fields = [gpu.KeyField(0, 4, "unsigned"), gpu.KeyField(4, 2, "signed", descending=True)]

    def records(n=4, width=8, dtype=torch.uint8, device="cuda"):
        return torch.zeros(n, width, dtype=dtype, device=device)

    _refused(gpu, name, f"{name} needs a tensor on a HIP device", records(device="cpu"), fields)
    part = "records must be a contiguous (n, R) uint8 tensor, one row per record"
    _refused(gpu, name, part, torch.zeros(32, dtype=torch.uint8, device="cuda"), fields)
    _refused(gpu, name, part, records(dtype=torch.int8), fields)
    _refused(gpu, name, part, records(width=16)[:, ::2], fields)
    _refused(gpu, name, "a key description is a sequence of KeyField", records(), [fields[0], (4, 2, "signed")], exc=TypeError)
    table, nf = _field_table(fields)
    need = int(_lib.load().rdst_hip_sort_records_by_fields_scratch_bytes(4, 8, table, nf))
    assert need > 0
    part = f"scratch must be a contiguous tensor on the records' device with at least {need} bytes"
    _refused(gpu, name, part, records(), fields, scratch=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    _refused(gpu, name, part, records(), fields, scratch=torch.empty(need, dtype=torch.uint8))
    _refused(gpu, name, part, records(), fields, scratch=torch.empty(2 * need, dtype=torch.uint8, device="cuda")[::2])
    # unlike the [u8; N] wrappers these look at the scratch whatever the number of rows
    _refused(gpu, name, "scratch must be a contiguous tensor on the records' device", records(n=1), fields,
             scratch=torch.empty(max(need, 1), dtype=torch.uint8))
    gpu.device_status()


# ---- the blocking in-place entries ----

@pytest.mark.parametrize("name", (LOWMEM, PARTITION))
def test_in_place_keys(gpu, name):
    import torch
    part = f"{name} needs a contiguous 1-D tensor on a HIP device"
    _refused(gpu, name, part, _keys(device="cpu"))
    _refused(gpu, name, part, _keys().reshape(4, 2))
    _refused(gpu, name, part, _keys(16)[::2])
    _refused(gpu, name, "no device RadixKey mapping", torch.zeros(8, dtype=torch.float16, device="cuda"), exc=TypeError)
    gpu.device_status()


def test_lowmem_scratch(gpu):
    import torch
    part = "scratch must be a contiguous tensor of the same dtype and device"
    _refused(gpu, LOWMEM, part, _keys(), scratch=torch.zeros(65536, dtype=torch.float32, device="cuda"))
    _refused(gpu, LOWMEM, part, _keys(), scratch=torch.zeros(65536, dtype=torch.int32))
    _refused(gpu, LOWMEM, part, _keys(), scratch=torch.zeros(2 * 65536, dtype=torch.int32, device="cuda")[::2])
    # at most one key: the call returns before it looks at the scratch
    assert _accepted(gpu, LOWMEM, _keys(1), scratch=torch.zeros(8, dtype=torch.float32)) is None
    assert _accepted(gpu, LOWMEM, _keys(0), scratch=torch.zeros(8, dtype=torch.float32)) is None
    gpu.device_status()
