"""CPU-side checks of the device-length entries (rdst_hip_sort_device_devlen, rdst_hip_sort_pairs_device_devlen): exported
and declared, every argument error of the known-length twins comes back with the twin's code and message, in the twin's
order, with `capacity` in the place of `len`; the three errors of the length argument come after them and before any
device work; capacity <= 1 is a no-op with NULL everything.  The pointers are made up: a call that got as far as the
device would fault."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
NEW = ("rdst_hip_sort_device_devlen", "rdst_hip_sort_pairs_device_devlen")
vp = ctypes.c_void_p


def _pointers():
    """five made-up 'device' pointers, 16-byte aligned, into one host buffer whose bytes are checked afterwards"""
    buf = np.random.default_rng(3).integers(0, 256, size=5 * 4096 + 16, dtype=np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16
    return buf, [base + 4096 * i for i in range(5)]


def _keys(lib, twin, k, t, n, kb, kind, levels, length=None, lb=8):
    if twin:
        return lib.rdst_hip_sort_device(vp(k), vp(t), n, kb, kind, levels, None)
    return lib.rdst_hip_sort_device_devlen(vp(k), vp(t), n, vp(length), lb, kb, kind, levels, None)


def _pairs(lib, twin, k, v, tk, tv, n, kb, kind, levels, vb, length=None, lb=8):
    if twin:
        return lib.rdst_hip_sort_pairs_device(vp(k), vp(v), vp(tk), vp(tv), n, kb, kind, levels, vb, None)
    return lib.rdst_hip_sort_pairs_device_devlen(vp(k), vp(v), vp(tk), vp(tv), n, vp(length), lb, kb, kind, levels, vb, None)


def test_symbols_header_and_python_surface(hiplib):
    import rdst_amd
    from rdst_amd import _lib
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(hiplib, name) is not None and name + "(" in header
        assert getattr(hiplib, name).restype is ctypes.c_int
    assert len(hiplib.rdst_hip_sort_device_devlen.argtypes) == 9 and len(hiplib.rdst_hip_sort_pairs_device_devlen.argtypes) == 12
    assert "#define RDST_HIP_ABI_VERSION 2\n" in header and hiplib.rdst_hip_abi_version() == 2
    for name in ("sort_device_devlen_tensor", "sort_pairs_device_devlen_tensor"):
        assert name in rdst_amd.__all__ and callable(getattr(rdst_amd, name))
    hpp = open(os.path.join(ROOT, "include", "rdst.hpp")).read()
    assert "void sort_device_devlen(" in hpp and "void sort_pairs_device_devlen(" in hpp
    internal = open(os.path.join(ROOT, "rdst_amd", "csrc", "rdst_internal.h")).read()
    assert "int sort_slice_devlen_locked(" in internal and "int sort_pairs_slice_devlen_locked(" in internal


def test_keys_entry_argument_errors_are_the_twin_s(hiplib):
    buf, (k, t, _v, _tv, ln) = _pointers()
    before = buf.copy()
    calls = [
        (k, t, 8, 3, UNSIGNED, 3), (k, t, 8, 0, UNSIGNED, 0), (k, t, 8, 32, UNSIGNED, 32),       # widths nothing is built for
        (k, t, 8, 2, FLOAT, 2), (k, t, 8, 16, FLOAT, 16),                                       # float keys are f32 / f64
        (k, t, 8, 4, UNSIGNED, 0),                                                              # LEVELS == 0
        (k, t, 8, 4, SIGNED, 3), (k, t, 8, 8, SIGNED, 4), (k, t, 8, 1, UNSIGNED, 2),            # levels != width
        (k, t, 8, 4, BYTES_BE, 4),                                                              # [u8; N] keys: another entry
        (k, t, 8, 4, 4, 4), (k, t, 8, 4, -1, 4),                                                # unknown kind
        (None, t, 8, 4, UNSIGNED, 4), (None, t, 1, 4, UNSIGNED, 4),                             # null keys
        (k + 2, t, 8, 4, UNSIGNED, 4), (k + 8, t, 8, 16, UNSIGNED, 16), (k + 1, t, 1, 2, SIGNED, 2),   # key alignment
        (k, t, 1 << 36, 4, UNSIGNED, 4),                                                        # capacity too large
        (k, None, 8, 4, UNSIGNED, 4),                                                           # null tmp
        (k, t + 2, 8, 4, UNSIGNED, 4), (k, t + 8, 2, 16, SIGNED, 16),                           # tmp alignment
        # the order of colliding rules
        (None, None, 8, 3, UNSIGNED, 0), (k + 1, None, 8, 4, 9, 3), (None, None, 1 << 36, 4, UNSIGNED, 4), (k + 2, None, 1 << 36, 4, UNSIGNED, 4),
    ]
    want = [UNSUPPORTED] * 5 + [ARG] * 4 + [UNSUPPORTED] + [ARG] * 4 + [ALIGN] * 3 + [ARG, ARG, ALIGN, ALIGN, UNSUPPORTED, ARG, ARG, ALIGN]
    assert len(want) == len(calls)
    for args, status in zip(calls, want):
        assert _keys(hiplib, True, *args) == status, args
        msg = hiplib.rdst_hip_last_error()
        for length, lb in ((ln, 8), (ln, 4), (None, 8), (ln + 1, 8), (ln, 3)):          # whatever the length argument is
            assert _keys(hiplib, False, *args, length=length, lb=lb) == status, args
            assert hiplib.rdst_hip_last_error() == msg, args
    assert np.array_equal(buf, before)


def test_pairs_entry_argument_errors_are_the_twin_s(hiplib):
    buf, (k, t, v, tv, ln) = _pointers()
    before = buf.copy()
    calls = [(k, v, t, tv, 8, kb, UNSIGNED, kb, 4) for kb in (1, 2, 16, 0, 3, 5, 12, 32)]                  # key widths
    calls += [(k, v, t, tv, 8, kb, UNSIGNED, kb, vb) for kb in (4, 8) for vb in (0, 1, 2, 3, 5, 12, 16)]   # value widths
    calls += [(k, v, t, tv, 8, 2, FLOAT, 2, 4), (k, v, t, tv, 8, 4, UNSIGNED, 0, 4), (k, v, t, tv, 8, 8, SIGNED, 7, 8),
              (k, v, t, tv, 8, 4, BYTES_BE, 4, 4), (k, v, t, tv, 8, 4, 7, 4, 4),
              (None, v, t, tv, 8, 4, UNSIGNED, 4, 4), (k + 2, v, t, tv, 8, 4, UNSIGNED, 4, 4), (k + 4, v, t, tv, 8, 8, UNSIGNED, 8, 4),
              (k, v, t, tv, 1 << 36, 4, UNSIGNED, 4, 4),
              (k, None, t, tv, 8, 4, UNSIGNED, 4, 4), (k, v, None, tv, 8, 4, UNSIGNED, 4, 4), (k, v, t, None, 1000, 4, UNSIGNED, 4, 4),
              (k, v, t + 2, tv, 8, 4, SIGNED, 4, 4), (k, v, t + 4, tv, 8, 8, SIGNED, 8, 4), (k, v + 2, t, tv, 8, 4, SIGNED, 4, 4),
              (k, v, t, tv + 4, 8, 4, SIGNED, 4, 8),
              # the order of colliding rules (tests/test_pairs_abi.py)
              (k, v, t, tv, 8, 3, UNSIGNED, 0, 4), (k, v, t, tv, 8, 2, UNSIGNED, 0, 4), (k, v, t, tv, 8, 4, BYTES_BE, 3, 4),
              (None, v, t, tv, 8, 4, 9, 4, 4), (k + 8, v, t, tv, 8, 16, UNSIGNED, 16, 4), (k + 2, v, t, tv, 8, 4, UNSIGNED, 4, 3),
              (k, v, t, tv, 1, 2, UNSIGNED, 2, 4), (k, None, None, None, 0, 4, UNSIGNED, 4, 16), (None, None, None, None, 1, 4, UNSIGNED, 4, 4),
              (k, None, t + 2, tv, 8, 4, UNSIGNED, 4, 4), (k, v + 2, t + 2, tv, 8, 4, UNSIGNED, 4, 4)]
    seen = set()
    for args in calls:
        status = _pairs(hiplib, True, *args)
        assert status != OK, args
        seen.add(status)
        msg = hiplib.rdst_hip_last_error()
        for length, lb in ((ln, 8), (ln, 4), (None, 4), (ln + 2, 4), (ln, 16)):
            assert _pairs(hiplib, False, *args, length=length, lb=lb) == status, args
            assert hiplib.rdst_hip_last_error() == msg, args
    assert seen == {ARG, UNSUPPORTED, ALIGN}
    assert np.array_equal(buf, before)


def test_length_argument_errors(hiplib):
    """after every check of the twins, before any device work: NULL, a width other than 4 or 8, a misaligned pointer — in
    that order"""
    buf, (k, t, v, tv, ln) = _pointers()
    before = buf.copy()
    entries = (lambda **kw: _keys(hiplib, False, k, t, 1000, 4, UNSIGNED, 4, **kw),
               lambda **kw: _keys(hiplib, False, k, t, 2, 16, SIGNED, 16, **kw),
               lambda **kw: _pairs(hiplib, False, k, v, t, tv, 1000, 8, FLOAT, 8, 4, **kw),
               lambda **kw: _pairs(hiplib, False, k, v, t, tv, 2, 4, UNSIGNED, 4, 8, **kw))
    for f in entries:
        for lb in (4, 8, 0, 3):
            assert f(length=None, lb=lb) == ARG and b"null length" in hiplib.rdst_hip_last_error()       # NULL before the width
        for lb in (0, 1, 2, 3, 5, 7, 12, 16, 0xFFFFFFFF):
            for length in (ln, ln + 1):                                                                   # the width before the alignment
                assert f(length=length, lb=lb) == ARG and b"4- or 8-byte" in hiplib.rdst_hip_last_error(), lb
        for length, lb in ((ln + 1, 4), (ln + 2, 4), (ln + 3, 4), (ln + 1, 8), (ln + 4, 8), (ln + 6, 8)):
            assert f(length=length, lb=lb) == ALIGN and b"length pointer" in hiplib.rdst_hip_last_error(), (length - ln, lb)
    assert np.array_equal(buf, before)


def test_capacity_up_to_one_is_a_no_op_with_null_everything(hiplib):
    buf, (k, t, v, tv, ln) = _pointers()
    before = buf.copy()
    for cap in (0, 1):
        for kb, kind in ((1, UNSIGNED), (2, SIGNED), (4, FLOAT), (8, FLOAT), (16, SIGNED)):
            for length, lb in ((None, 0), (None, 8), (ln + 1, 8), (ln, 3)):                                # dev_len is not looked at
                assert _keys(hiplib, False, k, None, cap, kb, kind, kb, length=length, lb=lb) == OK, (cap, kb)
                if cap == 0:
                    assert _keys(hiplib, False, None, None, cap, kb, kind, kb, length=length, lb=lb) == OK, (cap, kb)
        for kb in (4, 8):
            for vb in (4, 8):
                for length, lb in ((None, 0), (ln + 1, 4)):
                    assert _pairs(hiplib, False, k, None, None, None, cap, kb, FLOAT, kb, vb, length=length, lb=lb) == OK, (cap, kb, vb)
        assert _pairs(hiplib, False, k, v + 1, t + 1, tv + 1, cap, 8, UNSIGNED, 8, 8, length=None, lb=0) == OK
    assert _pairs(hiplib, False, None, None, None, None, 0, 4, UNSIGNED, 4, 4, length=None, lb=0) == OK
    assert np.array_equal(buf, before)


def test_devlen_cpp_source_compiles_and_links(tmp_path, hiplib):
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_devlen.cpp")
    exe = str(tmp_path / "test_rdst_devlen")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)
