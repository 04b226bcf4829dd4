"""CPU-side checks of the device-offsets segmented entries (rdst_hip_sort_segments_device_offsets,
rdst_hip_sort_segments_pairs_device_offsets, their scratch size and the plan hook): the symbols are exported and declared,
the ABI version stays 2, the scratch size is a pure function of n_segments, and every argument error returns before any
device work with the status the header names (host memory stands in for device pointers: no call below gets as far as a
device)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
INT_SYMBOLS = ("rdst_hip_sort_segments_device_offsets", "rdst_hip_sort_segments_pairs_device_offsets", "rdst_hip_debug_segments_plan_device")
SIZE_SYMBOL = "rdst_hip_sort_segments_device_offsets_scratch_bytes"
MAX_SEGMENTS = 1 << 30
vp = ctypes.c_void_p


def _pointers(count=6):
    """made-up 'device' pointers, 256-byte aligned, 64 KiB each"""
    bufs = [(ctypes.c_uint8 * (65536 + 256))() for _ in range(count)]
    ptrs = [(ctypes.cast(b, vp).value + 255) // 256 * 256 for b in bufs]
    return bufs, ptrs


def _need(lib, nseg):
    return int(lib.rdst_hip_sort_segments_device_offsets_scratch_bytes(nseg))


def _keys(lib, k, t, tmp_elems, n, off, ob, nseg, kb, kind, levels, scratch, sbytes):
    return lib.rdst_hip_sort_segments_device_offsets(vp(k), vp(t), tmp_elems, n, vp(off), ob, nseg, kb, kind, levels, vp(scratch), sbytes, None)


def _pairs(lib, k, v, tk, tv, tmp_elems, n, off, ob, nseg, kb, kind, levels, vb, scratch, sbytes):
    return lib.rdst_hip_sort_segments_pairs_device_offsets(vp(k), vp(v), vp(tk), vp(tv), tmp_elems, n, vp(off), ob, nseg, kb, kind, levels, vb,
                                                           vp(scratch), sbytes, None)


def _failed(lib, rc, code, word=None):
    msg = lib.rdst_hip_last_error()
    assert rc == code, (rc, code, msg)
    assert msg, "an error without a message"
    if word:
        assert word in msg, msg
    return True


def test_symbols_header_and_version(hiplib):
    from rdst_amd import _lib
    with open(os.path.join(ROOT, "include", "rdst_hip.h")) as f:
        header = f.read()
    for name in INT_SYMBOLS:
        assert hasattr(hiplib, name), name
        assert name in _lib.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert hasattr(hiplib, SIZE_SYMBOL) and SIZE_SYMBOL in _lib.SYMBOLS
    assert re.search(r"\buint64_t\s+" + SIZE_SYMBOL + r"\s*\(", header)
    assert header.count("src/sorter.rs:131-138") >= 4            # the segmented sort's citation, once more per new comment
    assert re.search(r"#define\s+RDST_HIP_ABI_VERSION\s+2\b", header)
    assert hiplib.rdst_hip_abi_version() == 2


def test_scratch_bytes_is_pure_and_monotone(hiplib):
    assert _need(hiplib, 0) == 0
    for n in (MAX_SEGMENTS + 1, 1 << 31, 1 << 40, (1 << 64) - 1):
        assert _need(hiplib, n) == 0, n
    rng = np.random.default_rng(5)
    ns = sorted({1, 2, 3, 15, 16, 17, 63, 64, 65, 1000, 70_001, MAX_SEGMENTS - 1, MAX_SEGMENTS}
                | {int(x) for x in rng.integers(1, MAX_SEGMENTS, size=200)} | {int(x) for x in rng.integers(1, 5000, size=200)})
    prev = 0
    for n in ns:
        b = _need(hiplib, n)
        assert b > 0 and b % 256 == 0 and b >= prev, n
        assert 32 * n <= b <= 48 * n + 4096, n                   # of the order the issue names: 32 to 48 bytes per segment and a header
        assert b == _need(hiplib, n)                             # the same answer twice
        prev = b
    import rdst_amd
    assert rdst_amd.segments_device_offsets_scratch_bytes(70_001) == _need(hiplib, 70_001)


def test_nothing_to_do_needs_no_pointers(hiplib):
    assert _keys(hiplib, None, None, 0, 0, None, 8, 0, 4, UNSIGNED, 4, None, 0) == OK
    assert _keys(hiplib, None, None, 0, 1000, None, 4, 0, 8, FLOAT, 8, None, 0) == OK
    assert _keys(hiplib, None, None, 0, 1000, None, 3, 0, 8, FLOAT, 8, None, 0) == OK        # no segment: nothing else is looked at
    assert _pairs(hiplib, None, None, None, None, 0, 0, None, 8, 0, 4, UNSIGNED, 4, 8, None, 0) == OK
    counts = (ctypes.c_uint64 * 3)(9, 9, 9)
    tmp_elems, flags = ctypes.c_uint64(9), ctypes.c_uint32(9)
    assert hiplib.rdst_hip_debug_segments_plan_device(None, 8, 0, 100, 4, 0, None, 0, None, 0, counts, ctypes.byref(tmp_elems),
                                                      ctypes.byref(flags), None) == OK
    assert list(counts) == [0, 0, 0] and tmp_elems.value == 0 and flags.value == 0


def test_errors_before_any_device_work(hiplib):
    _keep, (k, v, tk, tv, off, scr) = _pointers()
    nseg, n = 2, 30
    need = _need(hiplib, nseg)
    assert 0 < need <= 65536

    def keys(**kw):
        a = dict(k=k, t=None, tmp_elems=0, n=n, off=off, ob=8, nseg=nseg, kb=4, kind=UNSIGNED, levels=4, scratch=scr, sbytes=need)
        a.update(kw)
        return _keys(hiplib, **a)

    def pairs(**kw):
        a = dict(k=k, v=v, tk=None, tv=None, tmp_elems=0, n=n, off=off, ob=8, nseg=nseg, kb=4, kind=UNSIGNED, levels=4, vb=4, scratch=scr,
                 sbytes=need)
        a.update(kw)
        return _pairs(hiplib, **a)

    for call in (keys, pairs):
        # RDST_ERR_ARG
        assert _failed(hiplib, call(off=None), ERR_ARG, b"null offsets")
        for ob in (0, 1, 2, 3, 5, 16):
            assert _failed(hiplib, call(ob=ob), ERR_ARG, b"offset_bytes")
        assert _failed(hiplib, call(ob=4, n=1 << 32), ERR_ARG, b"2^32")
        assert _failed(hiplib, call(ob=4, n=(1 << 32) + 5), ERR_ARG, b"2^32")
        assert _failed(hiplib, call(scratch=None), ERR_ARG, b"null scratch")
        assert _failed(hiplib, call(sbytes=need - 1), ERR_ARG, b"scratch_bytes")
        assert _failed(hiplib, call(sbytes=0), ERR_ARG, b"scratch_bytes")
        # RDST_ERR_ALIGN
        assert _failed(hiplib, call(off=off + 4), ERR_ALIGN, b"offsets pointer")
        assert _failed(hiplib, call(off=off + 2, ob=4), ERR_ALIGN, b"offsets pointer")
        for shift in (4, 16, 128):
            assert _failed(hiplib, call(scratch=scr + shift, sbytes=need), ERR_ALIGN, b"scratch")
        # RDST_ERR_UNSUPPORTED
        assert _failed(hiplib, call(nseg=MAX_SEGMENTS + 1, sbytes=1 << 40), ERR_UNSUPPORTED, b"2^30")
    # tmp_elems > 0 with a NULL tmp
    assert _failed(hiplib, keys(tmp_elems=10, t=None), ERR_ARG, b"tmp")
    assert _failed(hiplib, pairs(tmp_elems=10, tk=None, tv=tv), ERR_ARG, b"tmp")
    assert _failed(hiplib, pairs(tmp_elems=10, tk=tk, tv=None), ERR_ARG, b"tmp")
    # a 4-byte aligned table of 4-byte offsets is fine as far as alignment goes (the next check answers)
    assert _failed(hiplib, keys(off=off + 4, ob=4, scratch=None), ERR_ARG, b"null scratch")
    # pair widths other than 4/8 x 4/8
    for kb in (1, 2, 16):
        assert _failed(hiplib, pairs(kb=kb, levels=kb), ERR_UNSUPPORTED, b"4- or 8-byte keys")
    for vb in (0, 1, 2, 3, 5, 12, 16):
        assert _failed(hiplib, pairs(vb=vb), ERR_UNSUPPORTED, b"values")
    # width, kind, levels, key pointer: as the host-offsets entries
    for kb in (0, 3, 5, 12, 32):
        assert _failed(hiplib, keys(kb=kb, levels=kb), ERR_UNSUPPORTED)
    assert _failed(hiplib, keys(kb=2, levels=2, kind=FLOAT), ERR_UNSUPPORTED)
    assert _failed(hiplib, keys(kind=BYTES_BE), ERR_UNSUPPORTED)
    assert _failed(hiplib, keys(kind=7), ERR_ARG, b"kind")
    assert _failed(hiplib, keys(levels=0), ERR_ARG, b"level")
    assert _failed(hiplib, keys(levels=3), ERR_ARG, b"levels")
    assert _failed(hiplib, keys(k=None), ERR_ARG, b"null key")
    assert _failed(hiplib, keys(k=k + 2), ERR_ALIGN)
    assert _failed(hiplib, keys(tmp_elems=10, t=tk + 2), ERR_ALIGN, b"tmp pointer")
    assert _failed(hiplib, pairs(v=None), ERR_ARG, b"null value")
    assert _failed(hiplib, pairs(v=v + 2), ERR_ALIGN, b"value pointer")


def test_plan_hook_checks_its_arguments(hiplib):
    _keep, (off, scr, *_rest) = _pointers()
    need = _need(hiplib, 2)
    counts = (ctypes.c_uint64 * 3)()
    tmp_elems, flags = ctypes.c_uint64(0), ctypes.c_uint32(0)

    def hook(off=off, ob=8, nseg=2, n=30, kb=4, vb=0, scratch=scr, sbytes=need, counts=counts, tmp=ctypes.byref(tmp_elems), fl=ctypes.byref(flags)):
        return hiplib.rdst_hip_debug_segments_plan_device(vp(off), ob, nseg, n, kb, vb, vp(scratch), sbytes, None, 0, counts, tmp, fl, None)

    assert _failed(hiplib, hook(off=None), ERR_ARG, b"null offsets")
    assert _failed(hiplib, hook(ob=2), ERR_ARG, b"offset_bytes")
    assert _failed(hiplib, hook(ob=4, n=1 << 32), ERR_ARG)
    assert _failed(hiplib, hook(off=off + 4), ERR_ALIGN)
    assert _failed(hiplib, hook(scratch=None), ERR_ARG)
    assert _failed(hiplib, hook(scratch=scr + 64), ERR_ALIGN)
    assert _failed(hiplib, hook(sbytes=need - 1), ERR_ARG)
    assert _failed(hiplib, hook(nseg=MAX_SEGMENTS + 1, sbytes=1 << 40), ERR_UNSUPPORTED)
    assert _failed(hiplib, hook(kb=3), ERR_UNSUPPORTED)
    assert _failed(hiplib, hook(kb=2, vb=4), ERR_UNSUPPORTED)
    assert _failed(hiplib, hook(counts=None), ERR_ARG, b"null output")
    assert _failed(hiplib, hook(fl=None), ERR_ARG, b"null output")
