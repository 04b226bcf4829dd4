"""CPU-side checks of the nowait segmented entries (rdst_hip_sort_segments_device_offsets_nowait,
rdst_hip_sort_segments_pairs_device_offsets_nowait and their scratch size): the symbols are exported and declared, the ABI
version stays 2, the scratch size is a pure function that is monotone in n_segments and in len and never below the plan's
own, and every argument error returns before any device work with the status the header names (host memory stands in for
device pointers: no call below gets as far as a device)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
INT_SYMBOLS = ("rdst_hip_sort_segments_device_offsets_nowait", "rdst_hip_sort_segments_pairs_device_offsets_nowait")
SIZE_SYMBOL = "rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes"
MAX_SEGMENTS = 1 << 30
WIDTHS = ((1, 0), (2, 0), (4, 0), (8, 0), (16, 0), (4, 4), (4, 8), (8, 4), (8, 8))
vp = ctypes.c_void_p


def _pointers(count=7):
    """made-up 'device' pointers, 256-byte aligned, 64 KiB each"""
    bufs = [(ctypes.c_uint8 * (65536 + 256))() for _ in range(count)]
    ptrs = [(ctypes.cast(b, vp).value + 255) // 256 * 256 for b in bufs]
    return bufs, ptrs


def _need(lib, nseg, n, kb=4, vb=0):
    return int(lib.rdst_hip_sort_segments_device_offsets_nowait_scratch_bytes(nseg, n, kb, vb))


def _old(lib, nseg):
    return int(lib.rdst_hip_sort_segments_device_offsets_scratch_bytes(nseg))


def _keys(lib, k, t, n, off, ob, nseg, kb, kind, levels, scratch, sbytes):
    return lib.rdst_hip_sort_segments_device_offsets_nowait(vp(k), vp(t), n, vp(off), ob, nseg, kb, kind, levels, vp(scratch), sbytes, None)


def _pairs(lib, k, v, tk, tv, n, off, ob, nseg, kb, kind, levels, vb, scratch, sbytes):
    return lib.rdst_hip_sort_segments_pairs_device_offsets_nowait(vp(k), vp(v), vp(tk), vp(tv), n, vp(off), ob, nseg, kb, kind, levels, vb, vp(scratch),
                                                                  sbytes, None)


def _failed(lib, rc, code, word=None):
    msg = lib.rdst_hip_last_error()
    assert rc == code, (rc, code, msg)
    assert msg, "an error without a message"
    if word:
        assert word in msg, msg
    return True


def test_symbols_header_and_version(hiplib):
    from rdst_amd import _lib
    import rdst_amd
    with open(os.path.join(ROOT, "include", "rdst_hip.h")) as f:
        header = f.read()
    for name in INT_SYMBOLS:
        assert hasattr(hiplib, name), name
        assert name in _lib.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert hasattr(hiplib, SIZE_SYMBOL) and SIZE_SYMBOL in _lib.SYMBOLS
    assert re.search(r"\buint64_t\s+" + SIZE_SYMBOL + r"\s*\(", header)
    for name in INT_SYMBOLS + (SIZE_SYMBOL,):       # each declaration's comment cites the reference's recursion over a chunk's buckets
        comment = header[:header.index(name + "(")].rsplit("/*", 1)[1]
        assert "src/sorter.rs:131-138" in comment, name
    assert re.search(r"RDST_STAGE_SEGMENTS_TILED\s*=\s*14\b", header) and _lib.RDST_STAGE_SEGMENTS_TILED == 14
    assert re.search(r"#define\s+RDST_HIP_ABI_VERSION\s+2\b", header)
    assert hiplib.rdst_hip_abi_version() == 2
    assert callable(rdst_amd.sort_segments_device_offsets_nowait_tensor) and callable(rdst_amd.segments_nowait_scratch_bytes)


def test_scratch_bytes_is_pure_and_monotone(hiplib):
    import rdst_amd
    top = (1 << 32) - 1
    for kb, vb in WIDTHS:
        assert _need(hiplib, 0, 1000, kb, vb) == 0
        for nseg in (MAX_SEGMENTS + 1, 1 << 31, 1 << 40, (1 << 64) - 1):
            assert _need(hiplib, nseg, 1000, kb, vb) == 0, nseg
        for n in (1 << 32, (1 << 32) + 1, 1 << 40, (1 << 64) - 1):
            assert _need(hiplib, 5, n, kb, vb) == 0, n
        assert _need(hiplib, 5, top, kb, vb) > 0 and _need(hiplib, MAX_SEGMENTS, top, kb, vb) > 0
    for kb, vb in ((0, 0), (3, 0), (5, 0), (12, 0), (32, 0), (1, 4), (2, 4), (16, 8), (4, 1), (4, 2), (4, 3), (8, 16), (4, 12)):
        assert _need(hiplib, 5, 1000, kb, vb) == 0, (kb, vb)
    rng = np.random.default_rng(7)
    nsegs = sorted({1, 2, 3, 63, 64, 65, 1000, 70_001, MAX_SEGMENTS} | {int(x) for x in rng.integers(1, MAX_SEGMENTS, size=12)}
                   | {int(x) for x in rng.integers(1, 5000, size=12)})
    lens = sorted({0, 1, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769, 10**6, top} | {int(x) for x in rng.integers(0, top, size=12)}
                  | {int(x) for x in rng.integers(0, 200_000, size=12)})
    for kb, vb in WIDTHS:
        lim = (ctypes.c_uint32 * 2)()
        assert hiplib.rdst_hip_sort_segments_limits(kb, vb, lim) == OK
        T = int(lim[1])
        table = [[_need(hiplib, s, n, kb, vb) for n in lens] for s in nsegs]
        for i, s in enumerate(nsegs):
            for j, n in enumerate(lens):
                b = table[i][j]
                assert b > 0 and b % 256 == 0, (s, n)
                assert b >= _old(hiplib, s), (s, n)                                  # the plan's layout is its first part
                assert i == 0 or b >= table[i - 1][j], (s, n)                       # monotone in n_segments
                assert j == 0 or b >= table[i][j - 1], (s, n)                       # monotone in len
                # the layout, restated: tile_base, digit_base and tile_counts behind the plan, each rounded up to 256 bytes
                n_long = min(s, n // (T + 1))
                tiles = n // T + n_long
                up = lambda x: -(-x // 256) * 256                                   # noqa: E731
                assert b == _old(hiplib, s) + up(4 * (n_long + 1)) + up(1024 * n_long) + up(1024 * tiles), (kb, vb, s, n)
        assert _need(hiplib, 70_001, 10**6, kb, vb) == _need(hiplib, 70_001, 10**6, kb, vb)            # the same answer twice
    # no segment can be long and no tile is full: the one word of tile_base and nothing else
    assert _need(hiplib, 100, 16383, 4, 0) == _old(hiplib, 100) + 256
    assert rdst_amd.segments_nowait_scratch_bytes(70_001, 10**6, "uint32") == _need(hiplib, 70_001, 10**6, 4, 0)
    assert rdst_amd.segments_nowait_scratch_bytes(70_001, 10**6, "uint64", 4) == _need(hiplib, 70_001, 10**6, 8, 4)


def test_nothing_to_do_needs_no_pointers(hiplib):
    assert _keys(hiplib, None, None, 0, None, 8, 0, 4, UNSIGNED, 4, None, 0) == OK
    assert _keys(hiplib, None, None, 1000, None, 4, 0, 8, FLOAT, 8, None, 0) == OK
    assert _keys(hiplib, None, None, 1 << 40, None, 3, 0, 8, FLOAT, 8, None, 0) == OK        # no segment: nothing else is looked at
    assert _pairs(hiplib, None, None, None, None, 0, None, 8, 0, 4, UNSIGNED, 4, 8, None, 0) == OK
    assert _pairs(hiplib, None, None, None, None, 1000, None, 8, 0, 8, SIGNED, 8, 4, None, 0) == OK


def test_errors_before_any_device_work(hiplib):
    _keep, (k, v, tk, tv, off, scr, _spare) = _pointers()
    nseg, n = 2, 30
    need = _need(hiplib, nseg, n)
    assert 0 < need <= 65536 and need == _need(hiplib, nseg, n, 4, 4)

    def keys(**kw):
        a = dict(k=k, t=tk, n=n, off=off, ob=8, nseg=nseg, kb=4, kind=UNSIGNED, levels=4, scratch=scr, sbytes=need)
        a.update(kw)
        return _keys(hiplib, **a)

    def pairs(**kw):
        a = dict(k=k, v=v, tk=tk, tv=tv, n=n, off=off, ob=8, nseg=nseg, kb=4, kind=UNSIGNED, levels=4, vb=4, scratch=scr, sbytes=need)
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
        # the plan's own size is not enough once a segment can be long
        big_n = 40_000
        assert _need(hiplib, nseg, big_n) > _old(hiplib, nseg)
        assert _failed(hiplib, call(n=big_n, sbytes=_old(hiplib, nseg)), ERR_ARG, b"scratch_bytes")
        assert _failed(hiplib, call(n=big_n, sbytes=_need(hiplib, nseg, big_n) - 1), ERR_ARG, b"nowait_scratch_bytes")
        # RDST_ERR_ALIGN
        assert _failed(hiplib, call(off=off + 4), ERR_ALIGN, b"offsets pointer")
        assert _failed(hiplib, call(off=off + 2, ob=4), ERR_ALIGN, b"offsets pointer")
        for shift in (4, 16, 128):
            assert _failed(hiplib, call(scratch=scr + shift, sbytes=need), ERR_ALIGN, b"scratch")
        # RDST_ERR_UNSUPPORTED
        assert _failed(hiplib, call(nseg=MAX_SEGMENTS + 1, sbytes=1 << 40), ERR_UNSUPPORTED, b"2^30")
        assert _failed(hiplib, call(n=1 << 32, sbytes=1 << 40), ERR_UNSUPPORTED, b"len below 2^32")          # (8-byte offsets)
        assert _failed(hiplib, call(n=(1 << 32) + 5, sbytes=1 << 40), ERR_UNSUPPORTED, b"len below 2^32")
    # a NULL tmp with len > 0 and n_segments > 0
    assert _failed(hiplib, keys(t=None), ERR_ARG, b"tmp")
    assert _failed(hiplib, pairs(tk=None, tv=tv), ERR_ARG, b"tmp")
    assert _failed(hiplib, pairs(tk=tk, tv=None), ERR_ARG, b"tmp")
    # a 4-byte aligned table of 4-byte offsets is fine as far as alignment goes (the next check answers)
    assert _failed(hiplib, keys(off=off + 4, ob=4, scratch=None), ERR_ARG, b"null scratch")
    # pair widths other than 4/8 x 4/8
    for kb in (1, 2, 16):
        assert _failed(hiplib, pairs(kb=kb, levels=kb), ERR_UNSUPPORTED, b"4- or 8-byte keys")
    for vb in (0, 1, 2, 3, 5, 12, 16):
        assert _failed(hiplib, pairs(vb=vb), ERR_UNSUPPORTED, b"values")
    # width, kind, levels, key pointer: as the other device entries
    for kb in (0, 3, 5, 12, 32):
        assert _failed(hiplib, keys(kb=kb, levels=kb), ERR_UNSUPPORTED)
    assert _failed(hiplib, keys(kb=2, levels=2, kind=FLOAT), ERR_UNSUPPORTED)
    assert _failed(hiplib, keys(kind=BYTES_BE), ERR_UNSUPPORTED)
    assert _failed(hiplib, keys(kind=7), ERR_ARG, b"kind")
    assert _failed(hiplib, keys(levels=0), ERR_ARG, b"level")
    assert _failed(hiplib, keys(levels=3), ERR_ARG, b"levels")
    assert _failed(hiplib, keys(k=None), ERR_ARG, b"null key")
    assert _failed(hiplib, keys(k=k + 2), ERR_ALIGN)
    assert _failed(hiplib, keys(t=tk + 2), ERR_ALIGN, b"tmp pointer")
    assert _failed(hiplib, pairs(tv=tv + 2), ERR_ALIGN, b"tmp value pointer")
    assert _failed(hiplib, pairs(v=None), ERR_ARG, b"null value")
    assert _failed(hiplib, pairs(v=v + 2), ERR_ALIGN, b"value pointer")
