"""CPU-side checks of the partial sort's entries (rdst_hip_topk_device, rdst_hip_topk_scratch_bytes, rdst_hip_topk_limits,
rdst_hip_debug_topk_state): exported and declared in every mirror, every argument error in the documented order — the key
arguments with the code and message of rdst_hip_sort_device —, the no-ops, and the two pure functions.  The pointers are made
up: a call that got as far as the device would fault; the bytes they point to are compared afterwards."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
LARGEST = 1
NEW = ("rdst_hip_topk_device", "rdst_hip_topk_scratch_bytes", "rdst_hip_topk_limits", "rdst_hip_debug_topk_state")
vp = ctypes.c_void_p
BIG = 1 << 40   # a scratch_bytes that is never too small


def _pointers():
    """four made-up 'device' pointers, 256-byte aligned, into one host buffer whose bytes are checked afterwards"""
    buf = np.random.default_rng(3).integers(0, 256, size=4 * 4096 + 256, dtype=np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    return buf, [base + 4096 * i for i in range(4)]


def _topk(lib, keys, n, k, out, idx, ib, scratch, sbytes, cap, kb, kind, levels, flags=0):
    return lib.rdst_hip_topk_device(vp(keys), n, k, vp(out), vp(idx), ib, vp(scratch), sbytes, cap, kb, kind, levels, flags, None)


def _need(lib, n, k, kb, ib, cap=0):
    return int(lib.rdst_hip_topk_scratch_bytes(n, k, kb, ib, cap))


def test_symbols_header_and_mirrors(hiplib):
    import rdst_amd
    from rdst_amd import _lib
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(hiplib, name) is not None and name + "(" in header
    assert hiplib.rdst_hip_topk_device.restype is ctypes.c_int and len(hiplib.rdst_hip_topk_device.argtypes) == 14
    assert hiplib.rdst_hip_topk_scratch_bytes.restype is ctypes.c_uint64
    assert "#define RDST_TOPK_LARGEST 1u\n" in header and _lib.RDST_TOPK_LARGEST == 1
    assert "RDST_STAGE_TOPK = 15" in header and _lib.RDST_STAGE_TOPK == 15
    assert "#define RDST_HIP_ABI_VERSION 2\n" in header and hiplib.rdst_hip_abi_version() == 2
    for name in ("topk_device_tensor", "topk_scratch_bytes", "topk_limits", "topk_state"):
        assert name in rdst_amd.__all__ and callable(getattr(rdst_amd, name))
    hpp = open(os.path.join(ROOT, "include", "rdst.hpp")).read()
    assert hpp.count("void topk_device(") == 2 and "template <typename T, typename Idx>\nvoid topk_device(" in hpp
    from rdst_amd import build as B
    assert any(s.endswith("rdst_topk.hip") for s in B.SOURCES)


def test_key_argument_errors_are_the_sort_s(hiplib):
    """step 1 (and 2): whatever the other arguments are"""
    buf, (k, o, i, s) = _pointers()
    before = buf.copy()
    calls = [
        (k, 8, 3, UNSIGNED, 3), (k, 8, 0, UNSIGNED, 0), (k, 8, 32, UNSIGNED, 32),                 # widths nothing is built for
        (k, 8, 2, FLOAT, 2), (k, 8, 16, FLOAT, 16),                                              # float keys are f32 / f64
        (k, 8, 4, UNSIGNED, 0),                                                                   # LEVELS == 0
        (k, 8, 4, SIGNED, 3), (k, 8, 8, SIGNED, 4), (k, 8, 1, UNSIGNED, 2),                       # levels != width
        (k, 8, 4, BYTES_BE, 4), (k, 8, 16, BYTES_BE, 16),                                         # [u8; N] keys
        (k, 8, 4, 4, 4), (k, 8, 4, -1, 4),                                                        # unknown kind
        (None, 8, 4, UNSIGNED, 4), (None, 1, 4, UNSIGNED, 4),                                     # null keys
        (k + 2, 8, 4, UNSIGNED, 4), (k + 8, 8, 16, UNSIGNED, 16), (k + 1, 1, 2, SIGNED, 2),       # key alignment
        (k, 1 << 36, 4, UNSIGNED, 4),                                                             # len too large
    ]
    want = [UNSUPPORTED] * 5 + [ARG] * 4 + [UNSUPPORTED] * 2 + [ARG] * 4 + [ALIGN] * 3 + [ARG]
    assert len(want) == len(calls)
    for (keys, n, kb, kind, levels), status in zip(calls, want):
        assert hiplib.rdst_hip_sort_device(vp(keys), vp(o), n, kb, kind, levels, None) == status
        msg = hiplib.rdst_hip_last_error()
        for rest in ((n + 1, None, None, 0, None, 0, 0, 6), (1, o, i, 4, s, BIG, 0, 0), (0, o + 1, i + 1, 3, s + 1, 0, 5, 0)):
            kk, out, idx, ib, scr, sb, cap, flags = rest
            assert _topk(hiplib, keys, n, kk, out, idx, ib, scr, sb, cap, kb, kind, levels, flags) == status
            assert hiplib.rdst_hip_last_error() == msg
    assert np.array_equal(buf, before)


def test_argument_errors_in_their_order(hiplib):
    buf, (k, o, i, s) = _pointers()
    before = buf.copy()
    n = 1000

    def call(keys=k, n=n, kk=10, out=o, idx=None, ib=0, scr=s, sb=BIG, cap=0, kb=4, kind=UNSIGNED, flags=0):
        return _topk(hiplib, keys, n, kk, out, idx, ib, scr, sb, cap, kb, kind, kb, flags), hiplib.rdst_hip_last_error()

    # 3: len >= 2^32, before k > len, unknown flags and every pointer
    for bad_n in (1 << 32, (1 << 36) - 1):
        assert call(n=bad_n, kk=bad_n + 1, flags=2, out=None, scr=None)[0] == UNSUPPORTED
    assert b"2^32" in hiplib.rdst_hip_last_error()
    # 4: k > len, before the flags and the no-op
    rc, msg = call(kk=n + 1, flags=2, out=None)
    assert rc == ARG and b"k is larger" in msg
    assert call(n=0, keys=None, kk=1)[0] == ARG
    # 5: unknown flag bits, before k == 0
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        rc, msg = call(kk=0, flags=flags, out=None, scr=None)
        assert rc == ARG and b"flag" in msg
    # 6: k == 0 is a no-op: nothing else is looked at
    for flags in (0, LARGEST):
        assert call(kk=0, out=None, idx=i + 1, ib=3, scr=None, sb=0, flags=flags)[0] == OK
        assert call(kk=0, out=o + 1, idx=None, ib=99, scr=s + 1, sb=0, kb=16, flags=flags)[0] == OK
        assert call(n=0, keys=None, kk=0, out=None, scr=None, sb=0, flags=flags)[0] == OK
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
    for ib in (0, 3, 99):                                                                        # keys only: any index_bytes
        assert call(idx=None, ib=ib, scr=None)[0] == ARG and b"null scratch" in hiplib.rdst_hip_last_error()
    # 12, 13, 14: the scratch
    rc, msg = call(scr=None, sb=0)
    assert rc == ARG and b"null scratch" in msg
    for off in (1, 16, 128, 255):
        rc, msg = call(scr=s + off, sb=0)
        assert rc == ALIGN and b"scratch not aligned" in msg
    for kb, ib, kk, cap in ((4, 0, 10, 0), (4, 4, 10, 0), (8, 8, 1000, 0), (16, 0, 1, 1), (1, 0, 500, 64), (4, 8, 1000, 5000)):
        need = _need(hiplib, n, kk, kb, ib, cap)
        assert need > 0
        for sb in (0, 1, need - 1):
            rc, msg = call(kk=kk, idx=i if ib else None, ib=ib, kb=kb, cap=cap, sb=sb)
            assert rc == ARG and b"rdst_hip_topk_scratch_bytes" in msg, (kb, ib, kk, cap, sb)
    assert np.array_equal(buf, before)


def test_scratch_bytes_is_pure_and_monotone(hiplib):
    f = hiplib.rdst_hip_topk_scratch_bytes
    for kb in (0, 3, 5, 12, 32):
        assert f(1000, 10, kb, 0, 0) == 0
    for kb in (1, 2, 16):
        assert f(1000, 10, kb, 4, 0) == 0 and f(1000, 10, kb, 8, 0) == 0 and f(1000, 10, kb, 0, 0) > 0
    for ib in (1, 2, 3, 16):
        assert f(1000, 10, 4, ib, 0) == 0
    for kb, ib in ((1, 0), (2, 0), (4, 0), (8, 0), (16, 0), (4, 4), (4, 8), (8, 4), (8, 8)):
        for n in (1, 1000, 10**6, 10**9, (1 << 32) - 1):
            ks = [k for k in (0, 1, 2, 100, 10**4, 10**6, n) if k <= n]
            caps = (0, 1, 2, 64, 4096, 1 << 20, 1 << 24)
            table = [[int(f(n, k, kb, ib, cap)) for cap in caps] for k in ks]
            assert table == [[int(f(n, k, kb, ib, cap)) for cap in caps] for k in ks]             # pure
            for row in table:
                assert all(v > 0 and v % 256 == 0 for v in row)
                assert row[1:] == sorted(row[1:])                                                 # monotone in cand_capacity (>= 1)
                assert row[0] == row[caps.index(1 << 20)]                                         # 0 = the default
            for a, b in zip(table, table[1:]):
                assert all(x <= y for x, y in zip(a, b))                                          # monotone in k
            assert f(n, ks[-1], kb, 4 if ib else 0, 0) == f(n, ks[-1], kb, 8 if ib else 0, 0)    # the index width costs nothing
    # what the layout promises: header, counters, two arrays of k and two of the capacity
    assert f(10**6, 1000, 4, 0, 4096) == 256 + 4 * 4096 + 2 * 4096 + 2 * 16384
    assert f(10**6, 1000, 4, 8, 4096) == 256 + 4 * 4096 + 2 * 8192 + 2 * 32768
    assert f(100, 100, 8, 0, 0) == 256 + 4 * 4096 + 4 * 1024                                      # the capacity never exceeds len


def test_limits_for_every_width(hiplib):
    out = (ctypes.c_uint32 * 3)()
    want = {1: (8, 1), 2: (12, 2), 4: (12, 3), 8: (12, 6), 16: (12, 11)}
    for kb, (digit, levels) in want.items():
        assert hiplib.rdst_hip_topk_limits(kb, 0, out) == OK and tuple(out) == (digit, 1 << 20, levels)
        for ib in (4, 8):
            rc = hiplib.rdst_hip_topk_limits(kb, ib, out)
            if kb in (4, 8):
                assert rc == OK and tuple(out) == (digit, 1 << 20, levels + 3)
            else:
                assert rc == UNSUPPORTED
        assert hiplib.rdst_hip_topk_limits(kb, 3, out) == ARG
    for kb in (0, 3, 32):
        assert hiplib.rdst_hip_topk_limits(kb, 0, out) == UNSUPPORTED
    assert hiplib.rdst_hip_topk_limits(4, 0, None) == ARG
    import rdst_amd
    assert rdst_amd.topk_limits("float32", 8) == (12, 1 << 20, 6) and rdst_amd.topk_limits("u128") == (12, 1 << 20, 11)
    assert rdst_amd.topk_scratch_bytes(10**6, 1000, "uint32", 0, 4096) == 256 + 4 * 4096 + 2 * 4096 + 2 * 16384


def test_the_k_selected_never_take_the_sort_that_waits():
    """k may be anything below 2^32, and rdst_hip_sort_device's route (sort_slice_locked -> sort_whole) splits slices from
    about 10^9 elements on counts it reads back on the host: the partial sort orders its k elements by the hook that is the
    pipeline alone"""
    import re
    csrc = os.path.join(ROOT, "rdst_amd", "csrc")
    topk = open(os.path.join(csrc, "rdst_topk.hip")).read()
    code = "\n".join(line.split("//")[0] for line in topk.splitlines())
    assert "sort_slice_nowait_locked(sel, sel_tmp, k," in code and "sort_slice_devlen_locked(cand, cand_tmp, cap," in code
    assert not re.search(r"\bsort_slice_locked\b", code) and "hipStreamSynchronize" not in code.split("rdst_hip_debug_topk_state")[0]
    assert "hipMemcpy" not in code.split("rdst_hip_debug_topk_state")[0]
    kernels = open(os.path.join(csrc, "rdst_kernels.hip")).read()
    body = kernels.split("int sort_slice_nowait_locked(")[1].split("\n}\n")[0]
    assert "run_pipeline<K, LV>(" in body and "sort_whole" not in body and "run_split_sort" not in body
    whole = kernels.split("int sort_whole(")[1].split("\n}\n")[0]
    assert "run_split_sort" in whole                      # (what the hook leaves out is still where this test says it is)
    assert "int sort_slice_nowait_locked(" in open(os.path.join(csrc, "rdst_internal.h")).read()
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    assert "This holds for every k up to len" in header and "index_bytes is not looked" in header


def test_topk_cpp_source_compiles_and_links(tmp_path, hiplib):
    import subprocess
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_topk.cpp")
    exe = str(tmp_path / "test_rdst_topk")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)


def test_state_hook_argument_errors(hiplib):
    out = (ctypes.c_uint64 * 4)()
    buf, (k, _o, _i, _s) = _pointers()
    assert hiplib.rdst_hip_debug_topk_state(None, None, out) == ARG
    assert hiplib.rdst_hip_debug_topk_state(vp(k), None, None) == ARG
    assert hiplib.rdst_hip_debug_topk_state(vp(k + 8), None, out) == ALIGN
