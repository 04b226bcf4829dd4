"""CPU-side checks of the order statistics' entries (rdst_hip_select_device, rdst_hip_select_scratch_bytes,
rdst_hip_select_limits, rdst_hip_debug_select_state): exported and declared in every mirror, every argument error in the
documented order — the key arguments with the code and message of rdst_hip_sort_device —, the no-op, and the two pure
functions.  The pointers are made up: a call that got as far as the device would fault; the bytes they point to are compared
afterwards."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
LARGEST = 1
NEW = ("rdst_hip_select_device", "rdst_hip_select_scratch_bytes", "rdst_hip_select_limits", "rdst_hip_debug_select_state")
vp = ctypes.c_void_p
BIG = 1 << 40   # a scratch_bytes that is never too small
FIXED = 256 + 2304 + 4 * 16384   # header, group table, counters


def _pointers():
    """four made-up 'device' pointers, 256-byte aligned, into one host buffer whose bytes are checked afterwards"""
    buf = np.random.default_rng(3).integers(0, 256, size=4 * 4096 + 256, dtype=np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    return buf, [base + 4096 * i for i in range(4)]


def _ranks(values):
    return None if values is None else (ctypes.c_uint64 * max(len(values), 1))(*values)


def _select(lib, keys, n, ranks, nr, out, idx, ib, scratch, sbytes, cap, kb, kind, levels, flags=0):
    return lib.rdst_hip_select_device(vp(keys), n, _ranks(ranks), nr, vp(out), vp(idx), ib, vp(scratch), sbytes, cap, kb, kind, levels, flags, None)


def _need(lib, n, nr, kb, ib, cap=0):
    return int(lib.rdst_hip_select_scratch_bytes(n, nr, kb, ib, cap))


def test_symbols_header_and_mirrors(hiplib):
    import rdst_amd
    from rdst_amd import _lib
    from rdst_amd import radix_sort
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(hiplib, name) is not None and name + "(" in header
    assert hiplib.rdst_hip_select_device.restype is ctypes.c_int and len(hiplib.rdst_hip_select_device.argtypes) == 15
    assert hiplib.rdst_hip_select_scratch_bytes.restype is ctypes.c_uint64
    assert "RDST_STAGE_SELECT = 16" in header and _lib.RDST_STAGE_SELECT == 16 and radix_sort.STAGE_NAMES[16] == "select"
    assert "#define RDST_HIP_ABI_VERSION 2\n" in header and hiplib.rdst_hip_abi_version() == 2
    for name in ("select_device_tensor", "select_scratch_bytes", "select_limits", "select_state", "quantile_ranks"):
        assert name in rdst_amd.__all__ and callable(getattr(rdst_amd, name))
    hpp = open(os.path.join(ROOT, "include", "rdst.hpp")).read()
    assert hpp.count("void select_device(") == 2 and "template <typename T, typename Idx>\nvoid select_device(" in hpp
    from rdst_amd import build as B
    assert any(s.endswith("rdst_select.hip") for s in B.SOURCES) and any(h.endswith("rdst_stream.h") for h in B.HEADERS)


def test_key_argument_errors_are_the_sort_s(hiplib):
    """steps 1 and 2: whatever the other arguments are"""
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
        for rest in (([n + 1], 1, None, None, 0, None, 0, 0, 6), ([0], 1, o, i, 4, s, BIG, 0, 0), (None, 0, o + 1, i + 1, 3, s + 1, 0, 5, 0)):
            ranks, nr, out, idx, ib, scr, sb, cap, flags = rest
            assert _select(hiplib, keys, n, ranks, nr, out, idx, ib, scr, sb, cap, kb, kind, levels, flags) == status
            assert hiplib.rdst_hip_last_error() == msg
    assert np.array_equal(buf, before)


def test_argument_errors_in_their_order(hiplib):
    buf, (k, o, i, s) = _pointers()
    before = buf.copy()
    n = 1000
    good = [0, 999, 500]

    def call(keys=k, n=n, ranks=good, nr=None, out=o, idx=None, ib=0, scr=s, sb=BIG, cap=0, kb=4, kind=UNSIGNED, flags=0):
        nr = (len(ranks) if ranks is not None else 0) if nr is None else nr
        return _select(hiplib, keys, n, ranks, nr, out, idx, ib, scr, sb, cap, kb, kind, kb, flags), hiplib.rdst_hip_last_error()

    # 3: len >= 2^32, before the flags, the ranks and every pointer
    for bad_n in (1 << 32, (1 << 36) - 1):
        rc, msg = call(n=bad_n, ranks=None, nr=3, flags=2, out=None, scr=None)
        assert rc == UNSUPPORTED and b"2^32" in msg
    # 4: unknown flag bits, before n_ranks == 0
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        rc, msg = call(ranks=None, nr=0, flags=flags, out=None, scr=None)
        assert rc == ARG and b"flag" in msg
    # 5: no ranks is a no-op: nothing else is looked at
    for flags in (0, LARGEST):
        assert call(ranks=None, nr=0, out=None, idx=i + 1, ib=3, scr=None, sb=0, flags=flags)[0] == OK
        assert call(ranks=[5000], nr=0, out=o + 1, idx=None, ib=99, scr=s + 1, sb=0, kb=16, flags=flags)[0] == OK
    # 6: NULL ranks
    rc, msg = call(ranks=None, nr=3, out=None, scr=None)
    assert rc == ARG and b"null ranks" in msg
    # 7: a rank that is not below len; the message names the first
    for ranks, first in (([1000], 0), ([0, 999, 1000, 5000], 2), ([5, 5, 5, 5, 1 << 40], 4), ([(1 << 64) - 1], 0)):
        rc, msg = call(ranks=ranks, out=None, scr=None)
        assert rc == ARG and f"ranks[{first}]".encode() in msg, msg
    # 8: the key output
    rc, msg = call(out=None, idx=i, ib=3, scr=None)
    assert rc == ARG and b"null key output" in msg
    for kb, off in ((2, 1), (4, 2), (8, 4), (16, 8)):
        rc, msg = call(out=o + off, kb=kb, idx=i, ib=3, scr=None)
        assert rc == ALIGN and b"key output" in msg
    # 9: the index output (only with an index: without one index_bytes is not looked at)
    for ib in (0, 1, 2, 3, 5, 16):
        rc, msg = call(idx=i + 1, ib=ib, kb=2, kind=SIGNED, scr=None)
        assert rc == ARG and b"index_bytes" in msg
    for kb in (1, 2, 16):
        for ib in (4, 8):
            rc, msg = call(idx=i + 1, ib=ib, kb=kb, scr=None)
            assert rc == UNSUPPORTED and b"an index output takes 4- or 8-byte keys" in msg
    for ib, off in ((4, 1), (4, 2), (8, 4), (8, 1)):
        rc, msg = call(idx=i + off, ib=ib, kb=8, kind=FLOAT, scr=None)
        assert rc == ALIGN and b"index output" in msg
    for ib in (0, 3, 99):                                                                        # keys only: any index_bytes
        assert call(idx=None, ib=ib, scr=None)[0] == ARG and b"null scratch" in hiplib.rdst_hip_last_error()
    # 10, 11, 12: the scratch
    rc, msg = call(scr=None, sb=0)
    assert rc == ARG and b"null scratch" in msg
    for off in (1, 16, 128, 255):
        rc, msg = call(scr=s + off, sb=0)
        assert rc == ALIGN and b"scratch not aligned" in msg
    for kb, ib, cap in ((4, 0, 0), (4, 4, 0), (8, 8, 0), (16, 0, 1), (1, 0, 64), (4, 8, 5000)):
        need = _need(hiplib, n, 3, kb, ib, cap)
        assert need > 0
        for sb in (0, 1, need - 1):
            rc, msg = call(idx=i if ib else None, ib=ib, kb=kb, cap=cap, sb=sb)
            assert rc == ARG and b"rdst_hip_select_scratch_bytes" in msg, (kb, ib, cap, sb)
    assert np.array_equal(buf, before)


def test_scratch_bytes_is_pure_monotone_and_never_len_sized(hiplib):
    f = hiplib.rdst_hip_select_scratch_bytes
    for kb in (0, 3, 5, 12, 32):
        assert f(1000, 10, kb, 0, 0) == 0
    for kb in (1, 2, 16):
        assert f(1000, 10, kb, 4, 0) == 0 and f(1000, 10, kb, 8, 0) == 0 and f(1000, 10, kb, 0, 0) > 0
    for ib in (1, 2, 3, 16):
        assert f(1000, 10, 4, ib, 0) == 0
    default = 1 << 24
    for kb, ib in ((1, 0), (2, 0), (4, 0), (8, 0), (16, 0), (4, 4), (4, 8), (8, 4), (8, 8)):
        elem = kb * (2 if ib else 1)
        caps = (0, 1, 2, 64, 4096, 1 << 20, default, 1 << 26)
        for n in (1, 1000, 10**6, 10**9, (1 << 32) - 1):
            row = [int(f(n, 64, kb, ib, cap)) for cap in caps]
            assert row == [int(f(n, 64, kb, ib, cap)) for cap in caps]                            # pure
            assert all(v > 0 and v % 256 == 0 for v in row)
            assert row[1:] == sorted(row[1:]) and row[0] == row[caps.index(default)]              # monotone; 0 = the default
            assert all(int(f(n, nr, kb, ib, 64)) == row[3] for nr in (0, 1, 65, 10**6))          # one round's worth, whatever n_ranks
            for cap, v in zip(caps, row):                                                         # what the layout promises
                c = min(cap or default, n)
                assert v == FIXED + 2 * ((c * elem + 255) // 256 * 256)
        for cap in (1, 64, 4096, default):                                                        # independent of len beyond the capacity
            assert len({int(f(n, 9, kb, ib, cap)) for n in (cap, cap + 1, 10**9, (1 << 32) - 1) if n >= cap}) == 1
        assert int(f((1 << 32) - 1, 64, kb, ib, 0)) == FIXED + 2 * default * elem                 # never len-sized
    import rdst_amd
    assert rdst_amd.select_scratch_bytes(10**9, 9, "uint32", 0, 4096) == FIXED + 2 * 16384
    assert rdst_amd.select_scratch_bytes(10**9, 9, "float64", 8, 4096) == FIXED + 2 * 65536


def test_limits_for_every_width(hiplib):
    out = (ctypes.c_uint32 * 5)()
    want = {1: (8, 1), 2: (12, 2), 4: (12, 4), 8: (12, 8), 16: (12, 16)}
    for kb, (digit0, levels) in want.items():
        assert hiplib.rdst_hip_select_limits(kb, 0, out) == OK and tuple(out) == (64, digit0, 8, 1 << 24, levels)
        for ib in (4, 8):
            rc = hiplib.rdst_hip_select_limits(kb, ib, out)
            if kb in (4, 8):
                assert rc == OK and tuple(out) == (64, digit0, 8, 1 << 24, levels + 4)
            else:
                assert rc == UNSUPPORTED
        assert hiplib.rdst_hip_select_limits(kb, 3, out) == ARG
    for kb in (0, 3, 32):
        assert hiplib.rdst_hip_select_limits(kb, 0, out) == UNSUPPORTED
    assert hiplib.rdst_hip_select_limits(4, 0, None) == ARG
    import rdst_amd
    assert rdst_amd.select_limits("float32", 8) == (64, 12, 8, 1 << 24, 8) and rdst_amd.select_limits("u128") == (64, 12, 8, 1 << 24, 16)


def test_no_wait_and_no_copy_outside_the_debug_hook():
    """the call is asynchronous for every input: the translation unit waits and copies in its blocking test hook alone, sorts
    its candidates by the hook whose length lives on the device, and shares the streaming reader with rdst_topk.hip instead of
    copying it"""
    csrc = os.path.join(ROOT, "rdst_amd", "csrc")
    select = open(os.path.join(csrc, "rdst_select.hip")).read()
    code = "\n".join(line.split("//")[0] for line in select.splitlines())
    body = code.split("rdst_hip_debug_select_state")[0]
    assert "rdst_hip_debug_select_state" in code and "int rdst_hip_select_device(" in body
    for banned in ("hipStreamSynchronize", "hipEventSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipStreamWaitEvent", "hipHostMalloc"):
        assert banned not in body, banned
    assert "sort_slice_devlen_locked(cand, cand_tmp, cap," in code and not re.search(r"\bsort_slice_locked\b", code)
    assert '#include "rdst_stream.h"' in select
    topk = open(os.path.join(csrc, "rdst_topk.hip")).read()
    shared = open(os.path.join(csrc, "rdst_stream.h")).read()
    assert '#include "rdst_stream.h"' in topk
    for name in ("void stream_keys(", "struct StreamCut", "KeyVec<K> load_vec(", "C compose(", "void flush_stage(", "void level_shape("):
        assert shared.count(name) == 1 and name not in topk and name not in select, name


def test_select_cpp_source_compiles_and_links(tmp_path, hiplib):
    import subprocess
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_select.cpp")
    exe = str(tmp_path / "test_rdst_select")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)


def test_state_hook_argument_errors(hiplib):
    out = (ctypes.c_uint64 * 4)()
    buf, (k, _o, _i, _s) = _pointers()
    assert hiplib.rdst_hip_debug_select_state(None, None, out) == ARG
    assert hiplib.rdst_hip_debug_select_state(vp(k), None, None) == ARG
    assert hiplib.rdst_hip_debug_select_state(vp(k + 8), None, out) == ALIGN
