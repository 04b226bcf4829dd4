"""The argument errors of the three segmented tensor wrappers (rdst_amd.sort_segments_device_tensor,
sort_segments_device_offsets_tensor, sort_segments_device_offsets_nowait_tensor): every operand the wrappers refuse raises a
ValueError that names what is wrong, before anything reaches the library.  A device is needed only because the wrappers
insist on device tensors: no call here gets as far as a sort, and device_status() stays clean."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOST, OFFSETS, NOWAIT = "sort_segments_device_tensor", "sort_segments_device_offsets_tensor", "sort_segments_device_offsets_nowait_tensor"
WRAPPERS = (HOST, OFFSETS, NOWAIT)
BORDERS = [0, 3, 8]


def _keys(key=None):
    import torch
    if key == "u128":
        return torch.arange(8, dtype=torch.int64, device="cuda").view(torch.uint64).reshape(4, 2)
    return torch.arange(8, 0, -1, dtype=torch.int32, device="cuda")


def _offsets(name, borders=BORDERS, device="cuda"):
    import torch
    return np.asarray(borders, dtype=np.int64) if name == HOST else torch.tensor(borders, dtype=torch.int64, device=device)


def _refused(gpu, name, part, keys, offsets=None, **kw):
    import torch
    before = keys.contiguous().clone()
    with pytest.raises(ValueError) as e:
        getattr(gpu, name)(keys, _offsets(name) if offsets is None else offsets, **kw)
    assert part in str(e.value), (name, str(e.value))
    assert torch.equal(before.view(torch.uint8), keys.contiguous().view(torch.uint8)), name


@pytest.mark.parametrize("name", WRAPPERS)
def test_keys(gpu, name):
    import torch
    _refused(gpu, name, f"{name} needs a tensor on a HIP device", _keys().cpu())
    _refused(gpu, name, "keys must be a contiguous 1-D tensor", _keys().reshape(4, 2))
    _refused(gpu, name, "keys must be a contiguous 1-D tensor", torch.arange(16, dtype=torch.int32, device="cuda")[::2])
    _refused(gpu, name, "a 128-bit key container has shape (n, 2)", _keys().view(torch.int64), key="u128")
    _refused(gpu, name, "keys must be a contiguous 1-D tensor", torch.zeros(4, 4, dtype=torch.int64, device="cuda").view(torch.uint64)[:, :2], key="u128")
    gpu.device_status()


@pytest.mark.parametrize("name", WRAPPERS)
def test_values(gpu, name):
    import torch
    part = "values must be a contiguous 1-D tensor of the keys' length on the keys' device"
    _refused(gpu, name, part, _keys(), values=torch.zeros(7, dtype=torch.int32, device="cuda"))
    _refused(gpu, name, part, _keys(), values=torch.zeros(8, dtype=torch.int32))
    _refused(gpu, name, part, _keys(), values=torch.zeros(4, 2, dtype=torch.int32, device="cuda"))
    _refused(gpu, name, part, _keys(), values=torch.zeros(16, dtype=torch.int32, device="cuda")[::2])
    # (4, 2) limbs are four keys: values count keys, not limbs (pairs of 16-byte keys are refused by the library, later)
    _refused(gpu, name, part, _keys("u128"), offsets=_offsets(name, [0, 1, 4]), values=torch.zeros(8, dtype=torch.int32, device="cuda"), key="u128")
    gpu.device_status()


def test_tmp_host_borders(gpu):
    """the host-borders wrapper looks at tmp only when a segment beyond block_max needs one"""
    import torch
    n = gpu.segments_limits("int32", 4)[1] + 1
    keys = torch.zeros(n + 3, dtype=torch.int32, device="cuda")
    values = torch.zeros(n + 3, dtype=torch.int32, device="cuda")
    off = np.asarray([0, 3, n + 3], dtype=np.int64)
    part = f"tmp must be a contiguous tensor of the keys' dtype and device with at least {n} keys"
    _refused(gpu, HOST, part, keys, offsets=off, tmp=torch.zeros(n, dtype=torch.float32, device="cuda"))
    _refused(gpu, HOST, part, keys, offsets=off, tmp=torch.zeros(n - 1, dtype=torch.int32, device="cuda"))
    _refused(gpu, HOST, part, keys, offsets=off, tmp=torch.zeros(n, dtype=torch.int32))
    _refused(gpu, HOST, part, keys, offsets=off, tmp=torch.zeros(2 * n, dtype=torch.int32, device="cuda")[::2])
    tmp = torch.zeros(n, dtype=torch.int32, device="cuda")
    part = f"tmp_values must be a contiguous tensor of the values' dtype and device with at least {n} elements"
    _refused(gpu, HOST, part, keys, offsets=off, tmp=tmp, values=values, tmp_values=torch.zeros(n, dtype=torch.int64, device="cuda"))
    _refused(gpu, HOST, part, keys, offsets=off, tmp=tmp, values=values, tmp_values=torch.zeros(n - 1, dtype=torch.int32, device="cuda"))
    gpu.device_status()


def test_tmp_device_offsets(gpu):
    """no length to check here: the longest segment is known only on the device (a short tmp is the library's to refuse)"""
    import torch
    part = "tmp must be a contiguous tensor of the keys' dtype and device"
    _refused(gpu, OFFSETS, part, _keys(), tmp=torch.zeros(8, dtype=torch.float32, device="cuda"))
    _refused(gpu, OFFSETS, part, _keys(), tmp=torch.zeros(8, dtype=torch.int32))
    _refused(gpu, OFFSETS, part, _keys(), tmp=torch.zeros(16, dtype=torch.int32, device="cuda")[::2])
    tmp, values = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    part = "tmp_values must be a contiguous tensor of the values' dtype and device"
    _refused(gpu, OFFSETS, part, _keys(), tmp=tmp, values=values, tmp_values=torch.zeros(8, dtype=torch.int64, device="cuda"))
    _refused(gpu, OFFSETS, part, _keys(), tmp=tmp, values=values, tmp_values=torch.zeros(8, dtype=torch.int32))
    _refused(gpu, OFFSETS, "tmp_values without tmp", _keys(), values=values, tmp_values=torch.zeros(8, dtype=torch.int32, device="cuda"))
    _refused(gpu, OFFSETS, "tmp_values without tmp", _keys(), tmp_values=torch.zeros(8, dtype=torch.int32, device="cuda"))
    gpu.device_status()


def test_tmp_nowait(gpu):
    import torch
    part = "tmp must be a contiguous tensor of the keys' dtype and device with at least as many elements"
    _refused(gpu, NOWAIT, part, _keys(), tmp=torch.zeros(8, dtype=torch.float32, device="cuda"))
    _refused(gpu, NOWAIT, part, _keys(), tmp=torch.zeros(7, dtype=torch.int32, device="cuda"))
    _refused(gpu, NOWAIT, part, _keys(), tmp=torch.zeros(8, dtype=torch.int32))
    _refused(gpu, NOWAIT, part, _keys("u128"), offsets=_offsets(NOWAIT, [0, 1, 4]), tmp=torch.zeros(3, 2, dtype=torch.int64, device="cuda").view(torch.uint64), key="u128")
    values = torch.zeros(8, dtype=torch.int32, device="cuda")
    part = "tmp_values must be a contiguous tensor of the values' dtype and device with at least as many elements"
    _refused(gpu, NOWAIT, part, _keys(), values=values, tmp_values=torch.zeros(8, dtype=torch.int64, device="cuda"))
    _refused(gpu, NOWAIT, part, _keys(), values=values, tmp_values=torch.zeros(7, dtype=torch.int32, device="cuda"))
    _refused(gpu, NOWAIT, "tmp_values without values", _keys(), tmp_values=torch.zeros(8, dtype=torch.int32, device="cuda"))
    gpu.device_status()


def test_offsets_host_borders(gpu):
    part = "offsets: a 1-D sequence of n_segments + 1 element indices"
    _refused(gpu, HOST, part, _keys(), offsets=np.asarray([[0, 3], [3, 8]]))
    _refused(gpu, HOST, part, _keys(), offsets=[])
    _refused(gpu, HOST, "offsets must be non-negative integers", _keys(), offsets=np.asarray([0.0, 3.0, 8.0]))
    _refused(gpu, HOST, "offsets must be non-negative integers", _keys(), offsets=[-1, 3, 8])
    gpu.device_status()


@pytest.mark.parametrize("name", (OFFSETS, NOWAIT))
def test_offsets_on_the_device(gpu, name):
    import torch
    _refused(gpu, name, "offsets must be a tensor on the keys' HIP device", _keys(), offsets=_offsets(name, device="cpu"))
    _refused(gpu, name, "offsets must be a tensor on the keys' HIP device", _keys(), offsets=BORDERS)
    part = "offsets: a contiguous 1-D tensor of n_segments + 1 element indices"
    _refused(gpu, name, part, _keys(), offsets=torch.tensor([[0, 3], [3, 8]], device="cuda"))
    _refused(gpu, name, part, _keys(), offsets=torch.empty(0, dtype=torch.int64, device="cuda"))
    _refused(gpu, name, part, _keys(), offsets=torch.tensor([0, 0, 3, 3, 8, 8], device="cuda")[::2])
    _refused(gpu, name, "offsets must be int32 or int64", _keys(), offsets=torch.tensor([0.0, 3.0, 8.0], device="cuda"))
    _refused(gpu, name, "offsets must be int32 or int64", _keys(), offsets=torch.tensor(BORDERS, dtype=torch.int16, device="cuda"))
    gpu.device_status()


@pytest.mark.parametrize("name", (OFFSETS, NOWAIT))
def test_scratch(gpu, name):
    import torch
    need = gpu.segments_device_offsets_scratch_bytes(2) if name == OFFSETS else gpu.segments_nowait_scratch_bytes(2, 8, "int32")
    assert need > 0
    part = f"scratch must be a contiguous tensor on the keys' device with at least {need} bytes"
    _refused(gpu, name, part, _keys(), scratch=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    _refused(gpu, name, part, _keys(), scratch=torch.empty(need, dtype=torch.uint8))
    _refused(gpu, name, part, _keys(), scratch=torch.empty(2 * need, dtype=torch.uint8, device="cuda")[::2])
    gpu.device_status()
