"""CPU-side checks of the nowait entries for wide keys (rdst_hip_sort_bytes_device_nowait,
rdst_hip_sort_records_by_fields_device_nowait): exported and declared, every argument error returns before any device work
with the blocking twin's code, in the twin's order, and the width cap of 128 bytes sits where the twin's cap does.  The
pointers are made up: a call that got as far as the device would fault."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
ARG, UNSUPPORTED, ALIGN = -1, -2, -6
MAX_N, NOWAIT_MAX_N = 4096, 128
NEW = ("rdst_hip_sort_bytes_device_nowait", "rdst_hip_sort_records_by_fields_device_nowait")


def _table(fields):
    from rdst_amd import _lib
    return (_lib.KeyFieldC * max(1, len(fields)))(*[_lib.KeyFieldC(*f) for f in fields]), len(fields)


def _buffers():
    buf = np.random.default_rng(5).integers(0, 256, size=8 * 5000, dtype=np.uint8)
    scratch = (ctypes.c_uint8 * 8192)()
    sp = ctypes.c_void_p((ctypes.cast(scratch, ctypes.c_void_p).value + 255) // 256 * 256)
    return buf, ctypes.c_void_p(buf.ctypes.data), scratch, sp


def test_symbols_header_and_python_surface(hiplib):
    import rdst_amd
    from rdst_amd import _lib
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(hiplib, name) is not None and name + "(" in header
    assert f"#define RDST_BYTES_NOWAIT_MAX_N {NOWAIT_MAX_N}u" in header and _lib.RDST_BYTES_NOWAIT_MAX_N == NOWAIT_MAX_N
    assert "#define RDST_HIP_ABI_VERSION 2\n" in header and hiplib.rdst_hip_abi_version() == 2
    for name in ("sort_bytes_device_nowait_tensor", "sort_records_device_nowait_tensor"):
        assert name in rdst_amd.__all__ and callable(getattr(rdst_amd, name))


def test_bytes_entry_argument_errors_are_the_twin_s(hiplib):
    buf, p, _scratch, sp = _buffers()
    before = buf.copy()
    twin, f = hiplib.rdst_hip_sort_bytes_device, hiplib.rdst_hip_sort_bytes_device_nowait
    need = hiplib.rdst_hip_sort_bytes_scratch_bytes(100, 20)
    calls = [
        (p, 8, 0, sp, 4096),                                     # N = 0
        (None, 8, 20, sp, 4096),                                 # null rows
        (p, 1 << 32, 20, sp, 1 << 62),                           # N > 16 needs len < 2^32
        (None, 1 << 32, 20, sp, 1 << 62),                        # ... and the null rows are seen first
        (p, 100, 20, None, 1 << 20),                             # null scratch
        (p, 100, 20, sp, need - 1),                              # scratch one byte short
        (p, 10, 17, ctypes.c_void_p(sp.value + 1), 1 << 20),     # scratch not 256-byte aligned
        (p, 100, 3, None, 1 << 20),                              # the forwarded widths check their scratch as well
        (p, 10, 16, ctypes.c_void_p(sp.value + 1), 1 << 20),
        (p, 1, 20, None, 0), (p, 0, NOWAIT_MAX_N, None, 0), (None, 0, 17, None, 0), (None, 1, 3, None, 0),   # len <= 1: no-op
    ]
    want = [ARG, ARG, UNSUPPORTED, ARG, ARG, ARG, ALIGN, ARG, ALIGN, 0, 0, 0, 0]
    for args, status in zip(calls, want):
        assert twin(*args, None) == status, args
        msg = hiplib.rdst_hip_last_error()
        assert f(*args, None) == status, args
        assert status == 0 or hiplib.rdst_hip_last_error() == msg, args
    assert f(p, 1 << 32, 20, sp, 1 << 62, None) == UNSUPPORTED and b"2^32" in hiplib.rdst_hip_last_error()
    assert np.array_equal(buf, before)


def test_bytes_entry_width_cap(hiplib):
    """N = 129 is refused where the twin refuses 4097: after N = 0, before the no-op lengths and every pointer check; the
    message names the blocking entry.  N = 128 passes the width check."""
    _buf, p, _scratch, sp = _buffers()
    f = hiplib.rdst_hip_sort_bytes_device_nowait
    for n_bytes in (NOWAIT_MAX_N + 1, 1000, MAX_N, MAX_N + 1, 0xFFFFFFFF):
        for rows, n, scratch in ((p, 8, sp), (None, 8, None), (None, 0, None), (p, 1, None), (p, 1 << 32, sp)):
            assert f(rows, n, n_bytes, scratch, 1 << 40, None) == UNSUPPORTED, (n_bytes, n)
            assert b"rdst_hip_sort_bytes_device" in hiplib.rdst_hip_last_error()
    assert hiplib.rdst_hip_sort_bytes_device(None, 8, NOWAIT_MAX_N + 1, sp, 1 << 40, None) == ARG       # the twin takes the width
    assert f(None, 8, NOWAIT_MAX_N, sp, 1 << 40, None) == ARG and b"rows" in hiplib.rdst_hip_last_error()
    assert f(p, 8, NOWAIT_MAX_N, sp, hiplib.rdst_hip_sort_bytes_scratch_bytes(8, NOWAIT_MAX_N) - 1, None) == ARG
    assert b"scratch" in hiplib.rdst_hip_last_error()
    assert f(p, 1, NOWAIT_MAX_N, None, 0, None) == 0


# the twin's table of description errors (tests/test_fields_abi.py), restated: every one is an error of the nowait entry too
BAD = [
    ("no fields", [], 16, ARG),
    ("17 fields", [(i % 16, 1, UNSIGNED, 0) for i in range(17)], 16, UNSUPPORTED),
    ("L past the twin's cap", [(0, 4096, BYTES_BE, 0), (0, 1, UNSIGNED, 0)], 4096, UNSUPPORTED),
    ("u24", [(0, 3, UNSIGNED, 0)], 16, UNSUPPORTED),
    ("i0", [(0, 0, SIGNED, 0)], 16, UNSUPPORTED),
    ("f16", [(0, 2, FLOAT, 0)], 16, UNSUPPORTED),
    ("empty byte string", [(0, 0, BYTES_BE, 0)], 16, UNSUPPORTED),
    ("byte string past the twin's cap", [(0, MAX_N + 1, BYTES_BE, 0)], 5000, UNSUPPORTED),
    ("unknown kind", [(0, 4, 4, 0)], 16, ARG),
    ("unknown flag", [(0, 4, UNSIGNED, 2)], 16, ARG),
    ("field past the record", [(13, 4, UNSIGNED, 0)], 16, ARG),
    ("offset overflow", [(0xFFFFFFFF, 8, UNSIGNED, 0)], 16, ARG),
    ("a bad field in a key that is too long as well", [(0, 100, BYTES_BE, 0), (100, 100, BYTES_BE, 2)], 200, ARG),
]


@pytest.mark.parametrize("what,fields,rec_bytes,status", BAD, ids=[b[0] for b in BAD])
def test_records_entry_description_errors_are_the_twin_s(hiplib, what, fields, rec_bytes, status):
    buf, p, _scratch, sp = _buffers()
    before = buf.copy()
    table, nf = _table(fields)
    twin, f = hiplib.rdst_hip_sort_records_by_fields_device, hiplib.rdst_hip_sort_records_by_fields_device_nowait
    for n in (8, 1, 0):                                              # an invalid description is an error at every length
        assert twin(p, n, rec_bytes, table, nf, sp, 1 << 40, None) == status, what
        msg = hiplib.rdst_hip_last_error()
        assert f(p, n, rec_bytes, table, nf, sp, 1 << 40, None) == status, what
        assert hiplib.rdst_hip_last_error() == msg
    assert np.array_equal(buf, before)


def test_records_entry_other_argument_errors_are_the_twin_s(hiplib):
    buf, p, _scratch, sp = _buffers()
    before = buf.copy()
    twin, f = hiplib.rdst_hip_sort_records_by_fields_device, hiplib.rdst_hip_sort_records_by_fields_device_nowait
    size = hiplib.rdst_hip_sort_records_by_fields_scratch_bytes
    for fields in ([(1, 2, UNSIGNED, 0), (4, 8, SIGNED, 1)], [(1, 2, UNSIGNED, 0)], [(0, 8, FLOAT, 0), (1, 15, BYTES_BE, 1)]):
        table, nf = _table(fields)
        need = size(100, 16, table, nf)
        assert need > 0
        calls = [
            (p, 8, 16, None, 2, sp, 4096),                           # null table
            (None, 8, 16, table, nf, sp, 4096),                      # null records
            (p, 1 << 32, 16, table, nf, sp, 1 << 62),                # len >= 2^32
            (p, 100, 16, table, nf, None, 1 << 20),                  # null scratch
            (p, 100, 16, table, nf, sp, need - 1),                   # scratch one byte short
            (p, 100, 16, table, nf, ctypes.c_void_p(sp.value + 16), 1 << 20),
            (None, 1, 16, table, nf, None, 0), (None, 0, 16, table, nf, None, 0),      # len <= 1: no-op before the pointer checks
        ]
        for args, status in zip(calls, [ARG, ARG, UNSUPPORTED, ARG, ARG, ALIGN, 0, 0]):
            assert twin(*args, None) == status, args
            msg = hiplib.rdst_hip_last_error()
            assert f(*args, None) == status, args
            assert status == 0 or hiplib.rdst_hip_last_error() == msg, args
    assert np.array_equal(buf, before)


def test_records_entry_width_cap(hiplib):
    """L = 129 is refused with the description errors (before the no-op lengths and the pointer checks), L = 128 is not"""
    _buf, p, _scratch, sp = _buffers()
    twin, f = hiplib.rdst_hip_sort_records_by_fields_device, hiplib.rdst_hip_sort_records_by_fields_device_nowait
    for fields in ([(0, 129, BYTES_BE, 0)], [(0, 128, BYTES_BE, 0), (3, 1, UNSIGNED, 1)], [(0, 16, UNSIGNED, 0)] * 8 + [(7, 1, SIGNED, 0)],
                   [(0, 4096, BYTES_BE, 0)]):
        table, nf = _table(fields)
        for rows, n, scratch in ((p, 8, sp), (None, 8, None), (None, 0, None), (None, 1, None), (p, 1 << 32, sp)):
            assert f(rows, n, 4096, table, nf, scratch, 1 << 40, None) == UNSUPPORTED, (fields, n)
            assert b"rdst_hip_sort_records_by_fields_device" in hiplib.rdst_hip_last_error()
        assert twin(None, 8, 4096, table, nf, sp, 1 << 40, None) == ARG                       # the twin takes the key
    for fields in ([(0, 128, BYTES_BE, 0)], [(0, 16, UNSIGNED, 0)] * 8, [(0, 127, BYTES_BE, 0), (3, 1, UNSIGNED, 1)]):
        table, nf = _table(fields)
        assert f(None, 8, 200, table, nf, sp, 1 << 40, None) == ARG and b"record" in hiplib.rdst_hip_last_error()
        assert f(None, 1, 200, table, nf, None, 0, None) == 0


def test_nowait_cpp_source_compiles_and_links(tmp_path, hiplib):
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_bytes_nowait.cpp")
    exe = str(tmp_path / "test_rdst_bytes_nowait")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)
