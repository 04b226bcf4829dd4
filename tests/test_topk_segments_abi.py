"""CPU-side checks of the segmented partial sort's entries (rdst_hip_topk_segments_device, ..._scratch_bytes, ..._limits,
rdst_topk_segments_plan, rdst_hip_set_topk_segments_stream_max): exported and declared in all three mirrors, every argument
error in the documented order — the shared arguments with rdst_hip_topk_device's codes —, the no-ops, and the pure
functions.  The pointers are made up: a call that got as far as the device would fault; the bytes they point to are compared
afterwards."""
import ctypes
import os

import numpy as np
import pytest

import topk_segments_inputs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
LARGEST = 1
NEW = ("rdst_hip_topk_segments_device", "rdst_hip_topk_segments_scratch_bytes", "rdst_hip_topk_segments_limits", "rdst_topk_segments_plan",
       "rdst_hip_set_topk_segments_stream_max")
WIDTHS = ((1, 0), (2, 0), (4, 0), (8, 0), (16, 0), (4, 4), (4, 8), (8, 4), (8, 8))
vp = ctypes.c_void_p
BIG = 1 << 40   # a scratch_bytes that is never too small


def _pointers():
    """four made-up 'device' pointers, 256-byte aligned, into one host buffer whose bytes are checked afterwards"""
    buf = np.random.default_rng(3).integers(0, 256, size=4 * 4096 + 256, dtype=np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    return buf, [base + 4096 * i for i in range(4)]


def _table(values):
    a = np.array(values, dtype=np.uint64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


@pytest.fixture
def setter(hiplib):
    yield hiplib.rdst_hip_set_topk_segments_stream_max
    hiplib.rdst_hip_set_topk_segments_stream_max(0)


def test_symbols_header_and_mirrors(hiplib):
    import rdst_amd
    from rdst_amd import _lib
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(hiplib, name) is not None and name + "(" in header
    assert hiplib.rdst_hip_topk_segments_device.restype is ctypes.c_int and len(hiplib.rdst_hip_topk_segments_device.argtypes) == 15
    assert hiplib.rdst_hip_topk_segments_scratch_bytes.restype is ctypes.c_uint64
    assert "#define RDST_HIP_ABI_VERSION 2\n" in header and hiplib.rdst_hip_abi_version() == 2
    for name in ("topk_segments_device_tensor", "topk_rows_tensor", "topk_segments_scratch_bytes", "topk_segments_limits", "topk_segments_plan"):
        assert name in rdst_amd.__all__ and callable(getattr(rdst_amd, name))
    hpp = open(os.path.join(ROOT, "include", "rdst.hpp")).read()
    assert hpp.count("void topk_segments(") == 2 and "template <typename T, typename Idx>\nvoid topk_segments(" in hpp
    from rdst_amd import build as B
    assert any(s.endswith("rdst_topk_segments.hip") for s in B.SOURCES)
    assert "no other copy to the host and no other wait" in header          # the asynchrony is stated where callers read it


def test_the_far_class_runs_on_the_hooks_that_never_wait():
    csrc = os.path.join(ROOT, "rdst_amd", "csrc")
    code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, "rdst_topk_segments.hip")).read().splitlines())
    assert "rdst_internal::topk_slice_locked(" in code and "rdst_internal::stage_segment_items(" in code
    for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipEventSynchronize", "sort_slice_locked"):
        assert word not in code, word
    topk = open(os.path.join(csrc, "rdst_topk.hip")).read()
    hook = topk.split("int rdst_internal::topk_slice_locked(")[1].split("\n}\n")[0]
    assert "return dispatch_topk(c);" in hook and "topk_layout(len, k, elem_bytes, index_bytes, 0)" in hook
    assert topk.count("pick_bucket(") == 1 and "pick_bucket(" in code     # one scan over the 4 096 counters, in rdst_device.h
    assert open(os.path.join(csrc, "rdst_device.h")).read().count("bool pick_bucket(") == 1


def test_limits_equal_the_layout_header(hiplib, setter):
    out = (ctypes.c_uint32 * 4)()
    layout = open(os.path.join(ROOT, "rdst_amd", "csrc", "rdst_segments_layout.h")).read()
    assert "constexpr uint32_t TOPK_STREAM_MAX_DEFAULT = 1u << 17;" in layout and S.STREAM_MAX_DEFAULT == 1 << 17
    seg = (ctypes.c_uint32 * 2)()
    for kb, ib in WIDTHS:
        assert hiplib.rdst_hip_topk_segments_limits(kb, ib, out) == OK
        assert hiplib.rdst_hip_sort_segments_limits(kb, 4 if ib else 0, seg) == OK    # the position is a u32 beside the key
        assert tuple(out) == (seg[0], seg[1], S.STREAM_MAX_DEFAULT, seg[1]) == S.limits(kb, bool(ib))
        for border in (1, seg[1] - 1, seg[1], seg[1] + 1, 1 << 22, (1 << 32) - 1):
            assert setter(border) == OK
            assert hiplib.rdst_hip_topk_segments_limits(kb, ib, out) == OK and tuple(out) == S.limits(kb, bool(ib), border)
            assert out[2] == max(border, seg[1])
        assert setter(0) == OK
    for kb in (1, 2, 16):
        for ib in (4, 8):
            assert hiplib.rdst_hip_topk_segments_limits(kb, ib, out) == UNSUPPORTED
    for kb in (0, 3, 32):
        assert hiplib.rdst_hip_topk_segments_limits(kb, 0, out) == UNSUPPORTED
    assert hiplib.rdst_hip_topk_segments_limits(4, 3, out) == ARG and hiplib.rdst_hip_topk_segments_limits(4, 0, None) == ARG
    import rdst_amd
    assert rdst_amd.topk_segments_limits("float32", 8) == (512, 16384, 1 << 17, 16384) and rdst_amd.topk_segments_limits("u128") == (256, 4096, 1 << 17, 4096)


def test_scratch_bytes_is_pure_monotone_and_moves_with_the_setter(hiplib, setter):
    f = hiplib.rdst_hip_topk_segments_scratch_bytes
    topk = hiplib.rdst_hip_topk_scratch_bytes
    for kb in (0, 3, 5, 32):
        assert f(10, 100, 5, kb, 0) == 0
    for kb in (1, 2, 16):
        assert f(10, 100, 5, kb, 4) == 0 and f(10, 100, 5, kb, 0) > 0
    assert f(0, 100, 5, 4, 0) == 0 and f(1 << 32, 100, 5, 4, 0) == 0 and f(10, 1 << 32, 5, 4, 0) == 0 and f(10, 100, 5, 4, 3) == 0
    for kb, ib in WIDTHS:
        _wm, bm, sm, _ksm = S.limits(kb, bool(ib))
        segs = (1, 2, 16, 17, 1000, 10**6, (1 << 32) - 1)
        longs = (0, 1, bm, bm + 1, sm, sm + 1, 1 << 24, (1 << 32) - 1)
        ks = (1, 64, bm, bm + 1, 1 << 21, 1 << 40)
        cube = [[[int(f(n, lg, k, kb, ib)) for k in ks] for lg in longs] for n in segs]
        assert cube == [[[int(f(n, lg, k, kb, ib)) for k in ks] for lg in longs] for n in segs]                   # pure
        for i, n in enumerate(segs):
            table = (16 * n + 255) // 256 * 256
            for j, lg in enumerate(longs):
                for m, k in enumerate(ks):
                    far = lg > sm or (lg > bm and k > bm)
                    assert cube[i][j][m] == table + (int(topk(lg, min(k, lg), kb, ib, 0)) if far else 0), (kb, ib, n, lg, k)
                    assert cube[i][j][m] % 256 == 0
                    if i: assert cube[i - 1][j][m] <= cube[i][j][m]                                                # monotone in all three
                    if j: assert cube[i][j - 1][m] <= cube[i][j][m]
                    if m: assert cube[i][j][m - 1] <= cube[i][j][m]
        # the setter moves the border the function uses
        lg = 4 * bm
        assert f(10, lg, 5, kb, ib) == 256
        assert setter(2 * bm) == OK
        assert f(10, lg, 5, kb, ib) == 256 + topk(lg, 5, kb, ib, 0) and f(10, 2 * bm, 5, kb, ib) == 256
        assert setter(0) == OK
        assert f(10, lg, 5, kb, ib) == 256
    import rdst_amd
    assert rdst_amd.topk_segments_scratch_bytes(17, 100, 5, "uint32") == 512


def _seg(lib, keys, n, off, nseg, k, out, idx, ib, scratch, sbytes, kb, kind, levels, flags=0):
    return lib.rdst_hip_topk_segments_device(vp(keys), n, off, nseg, k, vp(out), vp(idx), ib, vp(scratch), sbytes, kb, kind, levels, flags, None)


def test_key_argument_errors_are_the_partial_sort_s(hiplib):
    """steps 1 and 2, whatever the other arguments are: the code and message rdst_hip_topk_device gives"""
    buf, (k, o, i, s) = _pointers()
    before = buf.copy()
    _t, good = _table([0, 4, 8])
    calls = [
        (k, 8, 3, UNSIGNED, 3), (k, 8, 0, UNSIGNED, 0), (k, 8, 32, UNSIGNED, 32), (k, 8, 2, FLOAT, 2), (k, 8, 16, FLOAT, 16),
        (k, 8, 4, UNSIGNED, 0), (k, 8, 4, SIGNED, 3), (k, 8, 8, SIGNED, 4), (k, 8, 1, UNSIGNED, 2),
        (k, 8, 4, BYTES_BE, 4), (k, 8, 16, BYTES_BE, 16), (k, 8, 4, 4, 4), (k, 8, 4, -1, 4),
        (None, 8, 4, UNSIGNED, 4), (None, 1, 4, UNSIGNED, 4),
        (k + 2, 8, 4, UNSIGNED, 4), (k + 8, 8, 16, UNSIGNED, 16), (k + 1, 1, 2, SIGNED, 2),
        (k, 1 << 36, 4, UNSIGNED, 4),
    ]
    for keys, n, kb, kind, levels in calls:
        status = hiplib.rdst_hip_topk_device(vp(keys), n, 1, vp(o), None, 0, vp(s), BIG, 0, kb, kind, levels, 0, None)
        assert status != OK
        msg = hiplib.rdst_hip_last_error()
        for off, nseg, kk, out, idx, ib, scr, sb, flags in ((good, 2, 1, o, i, 4, s, BIG, 0), (None, 3, 9, None, None, 0, None, 0, 6), (good, 0, 0, o + 1, i + 1, 3, s + 1, 0, 0)):
            assert _seg(hiplib, keys, n, off, nseg, kk, out, idx, ib, scr, sb, kb, kind, levels, flags) == status
            assert hiplib.rdst_hip_last_error() == msg
    assert np.array_equal(buf, before)


def test_argument_errors_in_their_order(hiplib):
    buf, (k, o, i, s) = _pointers()
    before = buf.copy()
    n = 1000
    _t, good = _table([0, 10, 10, 700, 1000])
    _d, decreasing = _table([0, 10, 9, 700, 1000])
    _p, past = _table([0, 10, 10, 700, 1001])

    def call(keys=k, n=n, off=good, nseg=4, kk=10, out=o, idx=None, ib=0, scr=s, sb=BIG, kb=4, kind=UNSIGNED, flags=0):
        return _seg(hiplib, keys, n, off, nseg, kk, out, idx, ib, scr, sb, kb, kind, kb, flags), hiplib.rdst_hip_last_error()

    # 3: len >= 2^32, before the flags, the table and every pointer
    for bad_n in (1 << 32, (1 << 36) - 1):
        assert call(n=bad_n, flags=2, off=None, out=None, scr=None)[0] == UNSUPPORTED
    assert b"2^32" in hiplib.rdst_hip_last_error()
    # 4: unknown flag bits, before the no-ops
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        for kk, nseg in ((0, 4), (10, 0), (10, 4)):
            rc, msg = call(kk=kk, nseg=nseg, flags=flags, off=None, out=None, scr=None)
            assert rc == ARG and b"flag" in msg
    # 5: k == 0 or no segment is a no-op: nothing else is looked at; no limit on k
    for flags in (0, LARGEST):
        assert call(kk=0, off=None, out=None, idx=i + 1, ib=3, scr=None, sb=0, flags=flags)[0] == OK
        assert call(nseg=0, off=None, out=o + 1, idx=None, ib=99, scr=s + 1, sb=0, kb=16, flags=flags)[0] == OK
        assert call(kk=0, off=decreasing, out=None, scr=None, flags=flags)[0] == OK
    # 6: the table, before the outputs and the scratch
    rc, msg = call(off=None, out=None, scr=None)
    assert rc == ARG and b"null offsets" in msg
    rc, msg = call(nseg=1 << 32, out=None, scr=None)
    assert rc == ARG and b"n_segments" in msg
    rc, msg = call(off=decreasing, out=None, idx=i + 1, ib=3, scr=None)
    assert rc == ARG and b"non-decreasing" in msg
    rc, msg = call(off=past, out=None, scr=None, kk=1 << 40)
    assert rc == ARG and b"past len" in msg
    assert call(off=past, n=1001, scr=None)[0] == ARG and b"null scratch" in hiplib.rdst_hip_last_error()
    # 7, 8: the key output
    rc, msg = call(out=None, idx=i, ib=3, scr=None)
    assert rc == ARG and b"null key output" in msg
    for kb, off in ((2, 1), (4, 2), (8, 4), (16, 8)):
        rc, msg = call(out=o + off, kb=kb, idx=i, ib=3, scr=None)
        assert rc == ALIGN and b"key output" in msg
    # 9, 10, 11: the index output (only with an index: without one index_bytes is not looked at)
    for ib in (0, 1, 2, 3, 5, 16):
        rc, msg = call(idx=i + 1, ib=ib, kb=2, kind=SIGNED, scr=None)
        assert rc == ARG and b"index_bytes" in msg
    for kb in (1, 2, 16):
        for ib in (4, 8):
            rc, msg = call(idx=i + 1, ib=ib, kb=kb, scr=None)
            assert rc == UNSUPPORTED and b"4- or 8-byte keys" in msg
    for ib, off in ((4, 1), (4, 2), (8, 4), (8, 1)):
        rc, msg = call(idx=i + off, ib=ib, kb=8, kind=FLOAT, scr=None)
        assert rc == ALIGN and b"index output" in msg
    for ib in (0, 3, 99):
        assert call(idx=None, ib=ib, scr=None)[0] == ARG and b"null scratch" in hiplib.rdst_hip_last_error()
    # 12, 13, 14: the scratch; its need follows the table's longest segment (690 keys here) and k
    rc, msg = call(scr=None, sb=0)
    assert rc == ARG and b"null scratch" in msg
    for off in (1, 16, 128, 255):
        rc, msg = call(scr=s + off, sb=0)
        assert rc == ALIGN and b"scratch not aligned" in msg
    for kb, ib, kk in ((4, 0, 10), (4, 4, 10), (8, 8, 1000), (16, 0, 1), (1, 0, 1 << 40)):
        need = int(hiplib.rdst_hip_topk_segments_scratch_bytes(4, 690, kk, kb, ib))
        assert need == 256
        for sb in (0, 1, need - 1):
            rc, msg = call(kk=kk, idx=i if ib else None, ib=ib, kb=kb, sb=sb)
            assert rc == ARG and b"rdst_hip_topk_segments_scratch_bytes" in msg, (kb, ib, kk, sb)
    # a table of empty segments: everything is checked, nothing is done
    _e, empty = _table([5, 5, 5])
    assert call(off=empty, nseg=2, sb=255)[0] == ARG and call(off=empty, nseg=2, sb=256)[0] == OK
    assert np.array_equal(buf, before)


def test_a_far_segment_needs_its_part_of_the_scratch(hiplib, setter):
    """the need follows the class: a segment beyond the border set here, or beyond block_max with k beyond it, asks for
    rdst_hip_topk_scratch_bytes behind the table — checked before any device work"""
    buf, (k, o, _i, s) = _pointers()
    before = buf.copy()
    bm = S.block_max(4, False)
    n = 3 * bm
    _t, off = _table([0, 5, n])
    for border, kk in ((bm, 7), (0, bm + 1)):
        assert setter(border) == OK
        need = int(hiplib.rdst_hip_topk_segments_scratch_bytes(2, n - 5, kk, 4, 0))
        assert need == 256 + int(hiplib.rdst_hip_topk_scratch_bytes(n - 5, kk, 4, 0, 0))
        assert _seg(hiplib, k, n, off, 2, kk, o, None, 0, s, need - 1, 4, UNSIGNED, 4) == ARG
        assert b"rdst_hip_topk_segments_scratch_bytes" in hiplib.rdst_hip_last_error()
    assert np.array_equal(buf, before)


def test_cpp_source_compiles_and_links(tmp_path, hiplib):
    import subprocess
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_topk_segments.cpp")
    exe = str(tmp_path / "test_rdst_topk_segments")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)
