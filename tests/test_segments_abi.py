"""CPU-side checks of the segmented entries (rdst_hip_sort_segments_device, rdst_hip_sort_segments_pairs_device): the new
symbols are exported and declared, the ABI version stays 2, and every argument error returns before any device work with
the status the header names (host memory stands in for device pointers: no call below gets as far as a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
NEW_SYMBOLS = ("rdst_hip_sort_segments_device", "rdst_hip_sort_segments_pairs_device", "rdst_hip_sort_segments_limits", "rdst_segments_plan")


def _pointers():
    """four made-up 'device' pointers, 16-byte aligned"""
    bufs = [(ctypes.c_uint8 * 4096)() for _ in range(4)]
    ptrs = [(ctypes.cast(b, ctypes.c_void_p).value + 15) // 16 * 16 for b in bufs]
    return bufs, ptrs


def _offsets(values):
    a = np.ascontiguousarray(values, dtype=np.uint64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(a) - 1


def _keys(lib, k, t, tmp_elems, n, off, kb, kind, levels):
    vp = ctypes.c_void_p
    _keep, offp, nseg = _offsets(off) if off is not None else (None, None, 0)
    return lib.rdst_hip_sort_segments_device(vp(k), vp(t), tmp_elems, n, offp, nseg, kb, kind, levels, None)


def _pairs(lib, k, v, tk, tv, tmp_elems, n, off, kb, kind, levels, vb):
    vp = ctypes.c_void_p
    _keep, offp, nseg = _offsets(off) if off is not None else (None, None, 0)
    return lib.rdst_hip_sort_segments_pairs_device(vp(k), vp(v), vp(tk), vp(tv), tmp_elems, n, offp, nseg, kb, kind, levels, vb, None)


def _limits(lib, kb, vb):
    out = (ctypes.c_uint32 * 2)()
    assert lib.rdst_hip_sort_segments_limits(kb, vb, out) == OK
    return int(out[0]), int(out[1])


SHORT = [0, 10, 30]   # two wave-class segments


def test_symbols_header_and_version(hiplib):
    from rdst_amd import _lib
    with open(os.path.join(ROOT, "include", "rdst_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(hiplib, name), name
        assert name in _lib.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert "rdst_segment_item" in header and re.search(r"RDST_STAGE_SEGMENTS\s*=\s*13\b", header)
    assert re.search(r"#define\s+RDST_HIP_ABI_VERSION\s+2\b", header)
    assert hiplib.rdst_hip_abi_version() == 2


def test_nothing_to_do_needs_no_pointers(hiplib):
    assert _keys(hiplib, None, None, 0, 0, None, 4, UNSIGNED, 4) == OK
    assert _keys(hiplib, None, None, 0, 1000, None, 8, FLOAT, 8) == OK                  # no segment: len is not looked at
    assert _pairs(hiplib, None, None, None, None, 0, 0, None, 4, UNSIGNED, 4, 8) == OK
    _keep, (k, v, tk, tv) = _pointers()
    assert _keys(hiplib, k, None, 0, 100, [0, 0, 1, 1, 2], 4, SIGNED, 4) == OK         # lengths 0 and 1 only
    assert _pairs(hiplib, k, None, None, None, 0, 100, [5, 6, 6], 8, SIGNED, 8, 4) == OK


def test_width_kind_levels_as_the_slice_entries(hiplib):
    _keep, (k, v, tk, tv) = _pointers()
    for kb in (0, 3, 5, 12, 32):
        assert _keys(hiplib, k, tk, 0, 30, SHORT, kb, UNSIGNED, kb) == ERR_UNSUPPORTED, kb
        assert _pairs(hiplib, k, v, tk, tv, 0, 30, SHORT, kb, UNSIGNED, kb, 4) == ERR_UNSUPPORTED, kb
    for kb in (1, 2, 16):
        assert _keys(hiplib, k, tk, 0, 30, SHORT, kb, FLOAT, kb) == ERR_UNSUPPORTED                   # floats are f32 / f64
        assert _pairs(hiplib, k, v, tk, tv, 0, 30, SHORT, kb, UNSIGNED, kb, 4) == ERR_UNSUPPORTED     # a pair key width outside {4, 8}
        assert b"4- or 8-byte keys" in hiplib.rdst_hip_last_error()
    for kb in (4, 8):
        for vb in (0, 1, 2, 3, 5, 12, 16):
            assert _pairs(hiplib, k, v, tk, tv, 0, 30, SHORT, kb, UNSIGNED, kb, vb) == ERR_UNSUPPORTED, (kb, vb)
            assert b"values" in hiplib.rdst_hip_last_error()
        assert _keys(hiplib, k, tk, 0, 30, SHORT, kb, UNSIGNED, 0) == ERR_ARG                         # LEVELS == 0
        assert b"level" in hiplib.rdst_hip_last_error()
        for levels in (1, kb - 1, kb + 1):
            assert _keys(hiplib, k, tk, 0, 30, SHORT, kb, SIGNED, levels) == ERR_ARG, (kb, levels)
            assert _pairs(hiplib, k, v, tk, tv, 0, 30, SHORT, kb, SIGNED, levels, 4) == ERR_ARG, (kb, levels)
        assert _keys(hiplib, k, tk, 0, 30, SHORT, kb, BYTES_BE, kb) == ERR_UNSUPPORTED
        for kind in (4, 7, -1):
            assert _keys(hiplib, k, tk, 0, 30, SHORT, kb, kind, kb) == ERR_ARG, kind
            assert b"kind" in hiplib.rdst_hip_last_error()
            assert _pairs(hiplib, k, v, tk, tv, 0, 30, SHORT, kb, kind, kb, 8) == ERR_ARG, kind
    assert _keys(hiplib, None, tk, 0, 30, SHORT, 4, UNSIGNED, 4) == ERR_ARG
    assert b"null key" in hiplib.rdst_hip_last_error()
    assert _keys(hiplib, k, tk, 0, 1 << 36, SHORT, 4, UNSIGNED, 4) == ERR_ARG                         # len too large


def test_offsets(hiplib):
    _keep, (k, v, tk, tv) = _pointers()
    assert _keys(hiplib, k, tk, 0, 30, [0, 20, 10, 30], 4, UNSIGNED, 4) == ERR_ARG
    assert b"non-decreasing" in hiplib.rdst_hip_last_error()
    assert _keys(hiplib, k, tk, 0, 29, SHORT, 4, UNSIGNED, 4) == ERR_ARG
    assert b"past len" in hiplib.rdst_hip_last_error()
    vp = ctypes.c_void_p
    assert hiplib.rdst_hip_sort_segments_device(vp(k), vp(tk), 0, 30, None, 2, 4, UNSIGNED, 4, None) == ERR_ARG
    assert b"null offsets" in hiplib.rdst_hip_last_error()
    assert hiplib.rdst_hip_sort_segments_pairs_device(vp(k), vp(v), vp(tk), vp(tv), 0, 30, None, 2, 4, UNSIGNED, 4, 4, None) == ERR_ARG
    assert _pairs(hiplib, k, v, tk, tv, 0, 30, [0, 20, 10, 30], 8, FLOAT, 8, 4) == ERR_ARG


@pytest.mark.parametrize("kb,vb", [(1, 0), (4, 0), (8, 0), (16, 0), (4, 4), (8, 8)])
def test_long_segments_need_tmp(hiplib, kb, vb):
    _keep, (k, v, tk, tv) = _pointers()
    _wave_max, block_max = _limits(hiplib, kb, vb)
    longest = block_max + 9
    off = [0, 10, 10 + block_max + 1, 10 + block_max + 1 + longest]
    n = off[-1]

    def call(t, t2, tmp_elems):
        if vb == 0:
            return _keys(hiplib, k, t, tmp_elems, n, off, kb, UNSIGNED, kb)
        return _pairs(hiplib, k, v, t, t2, tmp_elems, n, off, kb, UNSIGNED, kb, vb)

    assert call(None, None, longest) == ERR_ARG                       # missing
    assert b"tmp" in hiplib.rdst_hip_last_error()
    assert call(tk, tv, longest - 1) == ERR_ARG                       # too small by one
    assert b"tmp_elems" in hiplib.rdst_hip_last_error()
    assert call(tk, tv, 0) == ERR_ARG
    if vb:
        assert call(tk, None, longest) == ERR_ARG                     # pairs: both scratch arrays


def test_alignment(hiplib):
    _keep, (k, v, tk, tv) = _pointers()
    assert _keys(hiplib, k + 2, tk, 0, 30, SHORT, 4, UNSIGNED, 4) == ERR_ALIGN
    assert _keys(hiplib, k + 8, tk, 0, 30, SHORT, 16, UNSIGNED, 16) == ERR_ALIGN
    assert _keys(hiplib, k, tk + 4, 30, 30, SHORT, 8, UNSIGNED, 8) == ERR_ALIGN
    assert b"tmp pointer" in hiplib.rdst_hip_last_error()
    assert _pairs(hiplib, k + 4, v, tk, tv, 30, 30, SHORT, 8, SIGNED, 8, 4) == ERR_ALIGN
    assert _pairs(hiplib, k, v + 2, tk, tv, 30, 30, SHORT, 4, SIGNED, 4, 4) == ERR_ALIGN
    assert b"value pointer" in hiplib.rdst_hip_last_error()
    assert _pairs(hiplib, k, v, tk + 2, tv, 30, 30, SHORT, 4, SIGNED, 4, 4) == ERR_ALIGN
    assert _pairs(hiplib, k, v, tk, tv + 4, 30, 30, SHORT, 4, SIGNED, 4, 8) == ERR_ALIGN
    assert _pairs(hiplib, k, None, tk, tv, 30, 30, SHORT, 4, SIGNED, 4, 8) == ERR_ARG
    assert b"null value" in hiplib.rdst_hip_last_error()
