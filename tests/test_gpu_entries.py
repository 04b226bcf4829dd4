"""The C ABI's entry points on a device: the argument answers that come after an entry's first HIP call (the ones before
it are in test_entry_abi.py), and what the blocking host-slice entries promise around the sort itself: the caller's
buffer is written only after the device reported success, a raised error word is reported once, the device the caller
had selected is selected again on return, and the cached device buffer of rdst_hip_sort grows and is reused.  The error
word is raised by the library's own debug hook (rdst_hip_debug_raise_device_error); nothing here faults."""
import ctypes
import math

import numpy as np
import pytest

from helpers import random_bits, reference_sorted, same_bits

pytestmark = pytest.mark.gpu

OK, ARG, ALIGN, DEVICE = 0, -1, -6, -5
U, S, F, BYTES_BE = 0, 1, 2, 3


@pytest.fixture()
def lib(gpu):
    from rdst_amd import _lib
    return _lib.load()


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _err(lib):
    return lib.rdst_hip_last_error()


def _raise_error_word(lib, device=None):
    import torch
    from rdst_amd import _lib
    with torch.cuda.device(device):
        _lib.check(lib.rdst_hip_debug_raise_device_error(2, _stream()))
        torch.cuda.synchronize()


def _opts(device=-1, low_memory=0):
    from rdst_amd import _lib
    return ctypes.byref(_lib.HipOptsC(device, low_memory, 0))


# ---- the host-slice entries: (input bytes, call, expected bytes) ------------------------------------------------------
def _ints(dtype, n, seed):
    a = random_bits(n, dtype, seed=seed).copy()
    kind = {"u": U, "i": S, "f": F}[a.dtype.kind]

    def call(lib, buf, opts):
        return lib.rdst_hip_sort(ctypes.c_void_p(buf.ctypes.data), n, a.dtype.itemsize, kind, a.dtype.itemsize, opts)
    return a, call, reference_sorted(a)


def _rows(nb, n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, nb), dtype=np.uint8)
    a[:, : nb - 1] &= 3                       # long common prefixes: the last bytes decide
    a[n // 2:] = a[: n - n // 2]              # and every row has a twin

    def call(lib, buf, opts):
        return lib.rdst_hip_sort(ctypes.c_void_p(buf.ctypes.data), n, nb, BYTES_BE, nb, opts)
    return a, call, a[np.lexsort(a.T[::-1])]


def _records(key_dtype, offset, n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, 24), dtype=np.uint8)
    kb = np.dtype(key_dtype).itemsize
    keys = rng.integers(-100, 100, n).astype(key_dtype)       # few values (u32: the negative ones wrap to the top): ties show the stable order
    a[:, offset: offset + kb] = keys.view(np.uint8).reshape(n, kb)
    kind = S if np.dtype(key_dtype).kind == "i" else U

    def call(lib, buf, opts):
        return lib.rdst_hip_sort_records(ctypes.c_void_p(buf.ctypes.data), n, 24, offset, kb, kind, opts)
    return a, call, a[np.argsort(keys, kind="stable")]


HOST_ENTRIES = {
    "sort u32": lambda: _ints("uint32", 10_000, 1),
    "sort f64": lambda: _ints("float64", 10_000, 2),
    "sort [u8; 3]": lambda: _rows(3, 5_000, 3),        # widened to 4-byte integers
    "sort [u8; 12]": lambda: _rows(12, 5_000, 4),      # widened to 16-byte integers
    "sort [u8; 40]": lambda: _rows(40, 5_000, 5),      # the rows route
    "records u32 @ 4": lambda: _records("uint32", 4, 5_000, 6),
    "records i64 @ 8": lambda: _records("int64", 8, 5_000, 7),
}


def _same(got, exp):
    return got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()


@pytest.mark.parametrize("entry", sorted(HOST_ENTRIES))
def test_host_entry_leaves_the_buffer_alone_on_failure_and_reports_once(lib, entry):
    raw, call, exp = HOST_ENTRIES[entry]()
    _raise_error_word(lib)
    got = raw.copy()
    assert call(lib, got, _opts()) == DEVICE and b"device error word = 0x2" in _err(lib)
    assert _same(got, raw)                                       # byte for byte the input
    assert call(lib, got, _opts()) == OK, _err(lib)              # reported once: the next call starts clean
    assert _same(got, exp)
    assert lib.rdst_hip_device_status(_stream()) == OK


@pytest.mark.parametrize("entry", ("sort u32", "sort [u8; 12]", "sort [u8; 40]", "records u32 @ 4"))
def test_host_entry_switches_back_to_the_callers_device(lib, entry):
    import torch
    raw, call, exp = HOST_ENTRIES[entry]()
    home = torch.cuda.current_device()
    try:
        # Another device than 0 where there is one.  With a single device `before` is 0, the device the entry is sent to, and
        # the current-device assertions below cannot fail; the rest of the test still holds.
        torch.cuda.set_device(torch.cuda.device_count() - 1)
        before = torch.cuda.current_device()
        got = raw.copy()
        assert call(lib, got, _opts(device=0)) == OK, _err(lib)
        assert torch.cuda.current_device() == before
        assert _same(got, exp)
        _raise_error_word(lib, device=0)
        assert torch.cuda.current_device() == before
        got = raw.copy()
        assert call(lib, got, _opts(device=0)) == DEVICE
        assert torch.cuda.current_device() == before
        assert _same(got, raw)
        assert call(lib, got, _opts(device=0)) == OK, _err(lib)
        assert _same(got, exp)
    finally:
        torch.cuda.set_device(home)


def test_host_timing_after_a_host_sort(lib):
    raw, call, exp = HOST_ENTRIES["sort u32"]()
    assert call(lib, raw, _opts()) == OK, _err(lib)
    t = [ctypes.c_float(-1) for _ in range(3)]
    assert lib.rdst_hip_host_timing(*(ctypes.byref(x) for x in t)) == OK, _err(lib)
    assert all(math.isfinite(x.value) and x.value >= 0 for x in t), [x.value for x in t]
    assert lib.rdst_hip_host_timing(None, None, None) == OK      # every output is optional


def test_low_memory_host_sort_takes_the_regions_route(lib):
    n = 200_000                                                  # scratch: 65 536 elements, so three tiles and a swap plan
    a = random_bits(n, "uint32", seed=11).copy()
    exp = reference_sorted(a)
    assert lib.rdst_hip_sort(ctypes.c_void_p(a.ctypes.data), n, 4, U, 4, _opts(low_memory=1)) == OK, _err(lib)
    assert same_bits(a, exp)


def test_lowmem_device_scratch_is_rounded_down_to_whole_4096s(lib):
    import torch
    n = 200_000
    a = random_bits(n, "uint32", seed=12).copy()
    keys = torch.from_numpy(a.view(np.int32)).cuda()
    tmp = torch.empty(69_631, dtype=torch.int32, device="cuda")  # rounds down to 65 536: accepted, and 65 536 are used
    tmp.fill_(0x5A5A5A5A)
    rc = lib.rdst_hip_sort_device_lowmem(ctypes.c_void_p(keys.data_ptr()), n, 4, U, 4, ctypes.c_void_p(tmp.data_ptr()), 69_631, _stream())
    assert rc == OK, _err(lib)
    assert same_bits(keys.cpu().numpy().view(np.uint32), reference_sorted(a))
    assert bool((tmp[65_536:] == 0x5A5A5A5A).all())


def test_cached_host_buffer_grows_and_is_reused(lib):
    for i, n in enumerate((1_000, 300_000, 1_000)):
        a = random_bits(n, "uint64", seed=20 + i).copy()
        exp = reference_sorted(a)
        assert lib.rdst_hip_sort(ctypes.c_void_p(a.ctypes.data), n, 8, U, 8, _opts()) == OK, _err(lib)
        assert same_bits(a, exp), n


# ---- argument answers behind the first HIP call ---------------------------------------------------------------------------
def test_null_outputs_of_the_readers(lib):
    n = ctypes.c_uint32(7)
    ms = (ctypes.c_float * 4)()
    st = (ctypes.c_uint32 * 4)()
    assert lib.rdst_hip_last_route(_stream(), None) == ARG and b"null output" in _err(lib)
    assert lib.rdst_hip_debug_last_sample(_stream(), None) == ARG and b"null output" in _err(lib)
    assert lib.rdst_hip_profile_run(0, None, 4, ctypes.byref(n)) == ARG and b"null output" in _err(lib)
    assert lib.rdst_hip_profile_run(0, ms, 4, None) == ARG and b"null output" in _err(lib)
    assert lib.rdst_hip_profile_run_stages(0, None, 4, ctypes.byref(n)) == ARG and b"null output" in _err(lib)
    assert lib.rdst_hip_profile_run_stages(0, st, 4, None) == ARG and b"null output" in _err(lib)
    assert n.value == 7


def test_no_such_profiled_run(lib):
    n = ctypes.c_uint32(7)
    ms = (ctypes.c_float * 4)()
    st = (ctypes.c_uint32 * 4)()
    try:
        assert lib.rdst_hip_set_profiling(1) == OK               # a fresh, empty record list
        assert lib.rdst_hip_profile_runs() == 0
        for run in (0, -1, 5):
            n.value = 7
            assert lib.rdst_hip_profile_run(run, ms, 4, ctypes.byref(n)) == ARG and b"no such profiled run" in _err(lib)
            assert n.value == 0
            n.value = 7
            assert lib.rdst_hip_profile_run_stages(run, st, 4, ctypes.byref(n)) == ARG and b"no such profiled run" in _err(lib)
            assert n.value == 0
        assert lib.rdst_hip_profile_run(0, None, 4, None) == ARG and b"null output" in _err(lib)   # the outputs before the run
    finally:
        lib.rdst_hip_set_profiling(0)


def test_split_entries_behind_their_memset(lib):
    import torch
    keys = torch.arange(1000, dtype=torch.int32, device="cuda")
    counts = torch.full((65536,), 9, dtype=torch.int64, device="cuda")
    kp, cp = ctypes.c_void_p(keys.data_ptr()), ctypes.c_void_p(counts.data_ptr())
    odd = ctypes.c_void_p(keys.data_ptr() + 2)
    # rdst_hip_split_top16_device clears its counts before it looks at len and tmp
    assert lib.rdst_hip_split_top16_device(kp, None, 1000, 4, U, cp, _stream()) == ARG and b"null tmp pointer" in _err(lib)
    torch.cuda.synchronize()
    assert int(counts.abs().sum()) == 0
    counts.fill_(9)
    assert lib.rdst_hip_split_top16_device(kp, odd, 1000, 4, U, cp, _stream()) == ALIGN and b"tmp pointer not aligned to the element size" in _err(lib)
    counts.fill_(9)
    assert lib.rdst_hip_split_top16_device(None, None, 0, 4, U, cp, _stream()) == OK, _err(lib)
    torch.cuda.synchronize()
    assert int(counts.abs().sum()) == 0
    # rdst_hip_split_top_level_device with len == 0: 256 zero counts, no dst asked for
    counts.fill_(9)
    assert lib.rdst_hip_split_top_level_device(None, None, 0, 4, U, cp, _stream()) == OK, _err(lib)
    torch.cuda.synchronize()
    assert int(counts[:256].abs().sum()) == 0 and bool((counts[256:] == 9).all())
    assert lib.rdst_hip_device_status(_stream()) == OK
