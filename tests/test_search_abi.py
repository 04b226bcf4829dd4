"""CPU-side checks of the binary search (rdst_hip_search_device, rdst_hip_search_scratch_bytes, rdst_hip_search_limits,
rdst_hip_debug_search_state): exported and declared in all three mirrors, the arity, every argument error in the documented
order with the sort's messages for the key arguments, the scratch-size function, the source check behind "no wait, no copy",
and the host-only half under the sanitizers.  The pointers are made up: a call that got as far as the device would fault; the
bytes they point to are compared afterwards."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rdst_amd", "csrc")
OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
NEW = ("rdst_hip_search_device", "rdst_hip_search_scratch_bytes", "rdst_hip_search_limits", "rdst_hip_debug_search_state")
vp = ctypes.c_void_p
BIG = 1 << 40   # a scratch_bytes that is never too small


def _pointers():
    """six made-up 'device' pointers, 256-byte aligned and 32 KiB apart, into one host buffer whose bytes are checked afterwards"""
    buf = np.random.default_rng(5).integers(0, 256, size=6 * 32768 + 256, dtype=np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    return buf, [base + 32768 * i for i in range(6)]


def _search(lib, hay, n, dlen, lb, needles, nn, lower, upper, ob, scratch, sbytes, kb, kind, levels, flags=0):
    return lib.rdst_hip_search_device(vp(hay), n, vp(dlen), lb, vp(needles), nn, vp(lower), vp(upper), ob, vp(scratch), sbytes, kb, kind, levels, flags, None)


def test_symbols_header_and_mirrors(hiplib):
    import rdst_amd
    from rdst_amd import _lib
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(hiplib, name) is not None and name + "(" in header
    assert hiplib.rdst_hip_search_device.restype is ctypes.c_int and len(hiplib.rdst_hip_search_device.argtypes) == 16
    declared = header.split("int rdst_hip_search_device(")[1].split(");")[0]
    assert declared.count(",") == 15                                              # the arity, as the header declares it
    assert hiplib.rdst_hip_search_scratch_bytes.restype is ctypes.c_uint64 and len(hiplib.rdst_hip_search_scratch_bytes.argtypes) == 3
    assert len(hiplib.rdst_hip_search_limits.argtypes) == 2 and len(hiplib.rdst_hip_debug_search_state.argtypes) == 3
    assert "#define RDST_HIP_ABI_VERSION 2\n" in header and hiplib.rdst_hip_abi_version() == 2
    for name in ("search_device_tensor", "search_scratch_bytes", "search_limits", "search_state", "unique_device_tensor"):
        assert name in rdst_amd.__all__ and callable(getattr(rdst_amd, name))
    hpp = open(os.path.join(ROOT, "include", "rdst.hpp")).read()
    assert hpp.count("void search_device(") == 1 and hpp.count("std::size_t search_scratch_bytes(") == 1
    assert "template <typename T, typename Off, typename Len = std::uint64_t>\nvoid search_device(" in hpp
    from rdst_amd import build as B
    for unit in ("rdst_search.hip", "rdst_search.cpp"):
        assert any(s.endswith(unit) for s in B.SOURCES)
    assert any(h.endswith("rdst_search_layout.h") for h in B.HEADERS)
    assert "fn rdst_hip_search_device(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    doc = " ".join(header.split("Binary search: the device twin")[1].split("int rdst_hip_search_device(")[0].replace(" * ", " ").split())
    assert "no copy to or from the host, no wait on an event or on the stream, no library workspace, no allocation" in doc
    assert "BIT-IDENTICAL" in doc and "THE ONLY DATA-DEPENDENT OUTCOME is that bit" in doc and "AN UNSORTED HAYSTACK costs correctness only, never safety" in doc
    for step in ("1. the key arguments", "2. RDST_KEY_BYTES_BE", "3. len or n_needles >= 2^32", "4. any flag bit", "5. with dev_len", "6. NULL dev_needles",
                 "7. offset_bytes", "8. both outputs NULL", "9. NULL scratch"):
        assert step in doc, step


def _code(name):
    return "\n".join(line.split("//")[0] for line in open(os.path.join(CSRC, name)).read().splitlines())


def test_the_entry_reaches_no_wait_and_no_copy():
    """in front of the blocking test hook the two translation units name no synchronise, no copy (the only direction there
    is from here would be to or from the host), no memset, no event, no pinned memory, no allocation and no hook that takes
    the library's workspace or sorts"""
    blocking = ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipMemset", "hipEventSynchronize", "hipStreamWaitEvent", "hipEventRecord",
                "hipHostMalloc", "hipMalloc", "workspace_take", "stage_segment_items", "sort_slice", "HostJob")
    hip = _code("rdst_search.hip")
    assert hip.count("rdst_hip_debug_search_state") == 1
    body, hook = hip.split('extern "C" int rdst_hip_debug_search_state')
    assert 'extern "C" int rdst_hip_search_device(' in body
    for code, unit in ((body, "rdst_search.hip"), (_code("rdst_search.cpp"), "rdst_search.cpp")):
        for word in blocking:
            assert word not in code, f"{word} in {unit}"
    assert hook.count("hipMemcpyAsync(") == 1 and hook.count("hipStreamSynchronize(") == 1             # the hook is the blocking one
    assert body.count("__global__") == 2 and body.count("rdst_internal::launch(") == 2
    assert "hip" not in _code("rdst_search.cpp").replace("rdst_hip", "").replace("rdst_kernels.hip", "").replace("rdst_search.hip", "")
    # positions: never (lo + hi) / 2; the key map is the shared one
    assert "lo[i] + (hi[i] - lo[i]) / 2" in body and "(lo[i] + hi[i]) / 2" not in body
    assert "map_key<K>(" in body and "map_key(K k" not in body and '#include "rdst_device.h"' in body


def test_scratch_bytes_and_limits(hiplib):
    import rdst_amd
    f = hiplib.rdst_hip_search_scratch_bytes
    for kb in (0, 3, 5, 32):
        assert f(10, 10, kb) == 0
    out = (ctypes.c_uint32 * 3)()
    assert hiplib.rdst_hip_search_limits(4, None) == ARG and hiplib.rdst_hip_search_limits(3, out) == UNSUPPORTED
    sizes = (0, 1, 2, 1023, 1024, 1025, 8192, 8193, 10**6, 10**9, (1 << 32) - 1)
    for kb in (1, 2, 4, 8, 16):
        assert hiplib.rdst_hip_search_limits(kb, out) == OK
        assert tuple(out) == ({1: 4096, 2: 2048, 4: 2048, 8: 2048, 16: 1024}[kb], 1024, {1: 8192, 2: 8192, 4: 8192, 8: 4096, 16: 2048}[kb])
        for big in (1 << 32, (1 << 64) - 1):
            assert f(big, 10, kb) == 0 and f(10, big, kb) == 0
        got = [[int(f(n, nn, kb)) for nn in sizes] for n in sizes]
        assert got == [[int(f(n, nn, kb)) for nn in sizes] for n in sizes]                          # pure
        for row in got:
            assert row == sorted(row)                                                             # monotone in n_needles
        for col in zip(*got):
            assert list(col) == sorted(col)                                                       # ... and in len
        assert all(x == 256 + 1024 * kb for row in got for x in row)                              # the header and the table
    assert rdst_amd.search_scratch_bytes(10**6, 10**6, "uint32") == 256 + 4096 and rdst_amd.search_scratch_bytes(0, 0, "u128") == 256 + 16384


def test_key_argument_errors_are_the_sort_s(hiplib):
    """step 1, whatever the other arguments are: the code and message rdst_hip_sort_device gives"""
    buf, (k, q, lo, up, x, t) = _pointers()
    before = buf.copy()
    calls = [(k, 8, 3, UNSIGNED, 3), (k, 8, 0, UNSIGNED, 0), (k, 8, 32, UNSIGNED, 32), (k, 8, 2, FLOAT, 2), (k, 8, 16, FLOAT, 16), (k, 8, 4, UNSIGNED, 0),
             (k, 8, 4, SIGNED, 3), (k, 8, 8, SIGNED, 4), (k, 8, 1, UNSIGNED, 2), (k, 8, 4, BYTES_BE, 4), (k, 8, 16, BYTES_BE, 16), (k, 8, 4, 4, 4),
             (k, 8, 4, -1, 4), (None, 8, 4, UNSIGNED, 4), (None, 1, 4, UNSIGNED, 4), (k + 2, 8, 4, UNSIGNED, 4), (k + 8, 8, 16, UNSIGNED, 16),
             (k + 1, 1, 2, SIGNED, 2), (k, 1 << 36, 4, UNSIGNED, 4)]
    for hay, n, kb, kind, levels in calls:
        status = hiplib.rdst_hip_sort_device(vp(hay), vp(t), n, kb, kind, levels, None)
        assert status != OK
        msg = hiplib.rdst_hip_last_error()
        for dlen, lb, needles, nn, lower, upper, ob, scr, sb, flags in ((None, 0, q, 8, lo, up, 8, x, BIG, 0), (k + 1, 3, None, 1 << 40, None, None, 3, None, 0, 6),
                                                                        (None, 0, q + 1, 0, k, k, 4, x + 1, 0, 1)):
            assert _search(hiplib, hay, n, dlen, lb, needles, nn, lower, upper, ob, scr, sb, kb, kind, levels, flags) == status
            assert hiplib.rdst_hip_last_error() == msg
    assert np.array_equal(buf, before)


def test_argument_errors_in_their_order(hiplib):
    buf, (k, q, lo, up, x, t) = _pointers()
    before = buf.copy()

    def call(hay=k, n=1000, dlen=None, lb=0, needles=q, nn=500, lower=lo, upper=up, ob=8, scr=x, sb=BIG, kb=4, kind=UNSIGNED, flags=0):
        return _search(hiplib, hay, n, dlen, lb, needles, nn, lower, upper, ob, scr, sb, kb, kind, kb, flags), hiplib.rdst_hip_last_error()

    bad = dict(dlen=t + 1, lb=3, needles=None, ob=3, lower=None, upper=None, scr=None)   # everything behind the step under test is wrong too
    # 3: len or n_needles >= 2^32 before the flags; 4: the flags before the length
    for kw in (dict(n=1 << 32), dict(nn=1 << 32), dict(nn=(1 << 64) - 1)):
        rc, msg = call(flags=2, **dict(bad, **kw))
        assert rc == UNSUPPORTED and b"2^32" in msg
    for flags in (1, 2, 3, 0x80000000):
        rc, msg = call(flags=flags, **bad)
        assert rc == ARG and b"flag" in msg
    # 5: the device-resident length, only when there is one
    for lb in (0, 1, 2, 3, 5, 16):
        rc, msg = call(**dict(bad, lb=lb))
        assert rc == ARG and b"device-resident length" in msg
    for lb, shift in ((4, 1), (4, 2), (8, 4), (8, 1)):
        rc, msg = call(**dict(bad, dlen=t + shift, lb=lb))
        assert rc == ALIGN and b"length pointer" in msg
    # 6: the needles (without dev_len, len_bytes is not looked at)
    rc, msg = call(**dict(bad, dlen=None, lb=99))
    assert rc == ARG and b"null needle pointer" in msg
    for kb, shift in ((2, 1), (4, 2), (8, 4), (16, 8)):
        rc, msg = call(**dict(bad, dlen=t, lb=4, needles=q + shift, kb=kb, n=100, nn=50))
        assert rc == ALIGN and b"needle pointer" in msg
    # 7: offset_bytes
    for ob in (0, 1, 2, 3, 5, 16):
        rc, msg = call(**dict(bad, dlen=None, needles=q, ob=ob))
        assert rc == ARG and b"offset_bytes" in msg
    # 8: the outputs: both NULL, alignment, overlap
    rc, msg = call(lower=None, upper=None, scr=None)
    assert rc == ARG and b"both outputs are null" in msg
    for ob, shift in ((4, 1), (4, 2), (8, 4), (8, 1)):
        rc, msg = call(lower=lo + shift, upper=k, ob=ob, scr=None)
        assert rc == ALIGN and b"lower output" in msg
        rc, msg = call(upper=up + shift, lower=k, ob=ob, scr=None)
        assert rc == ALIGN and b"upper output" in msg
    for kw in (dict(lower=k), dict(upper=k + 4 * 999 - 3996 % 8), dict(lower=k - 8 * 499), dict(upper=q), dict(lower=q + 4 * 499 - 4), dict(upper=q - 8 * 499),
               dict(dlen=t, lb=8, lower=t), dict(dlen=t + 4, lb=4, upper=t - 8 * 499)):
        rc, msg = call(scr=None, **kw)
        assert rc == ARG and b"an output overlaps" in msg, kw
    for kw in (dict(upper=lo), dict(upper=lo + 8 * 499), dict(lower=up + 8 * 499)):
        rc, msg = call(scr=None, **kw)
        assert rc == ARG and b"overlap each other" in msg, kw
    for kw in (dict(lower=k - 8 * 500), dict(lower=k + 4 * 1000), dict(upper=q + 4 * 500), dict(upper=lo + 8 * 500), dict(lower=None), dict(upper=None),
               dict(hay=q, n=500), dict(hay=q - 4 * 10, n=1000), dict(dlen=k, lb=4), dict(dlen=q, lb=8)):   # touching is no overlap; the inputs may overlap
        rc, msg = call(scr=None, **kw)
        assert rc == ARG and b"null scratch" in msg, kw
    # 9: the scratch
    for shift in (1, 16, 128, 255):
        rc, msg = call(scr=x + shift, sb=0)
        assert rc == ALIGN and b"scratch not aligned" in msg
    for kb, n, nn in ((4, 1000, 500), (1, 0, 1), (16, 100, 100), (8, (1 << 32) - 1, 1)):
        need = int(hiplib.rdst_hip_search_scratch_bytes(n, nn, kb))
        assert need == 256 + 1024 * kb
        for sb in (0, 1, 256, need - 1):
            rc, msg = call(n=n, nn=nn, kb=kb, sb=sb, hay=k if n else None, lower=k - 64 if n > 10**6 else lo, upper=None)
            assert rc == ARG and b"rdst_hip_search_scratch_bytes" in msg, (kb, n, sb)
    need = 256 + 4096
    for kw in (dict(scr=k), dict(scr=k - need + 256), dict(scr=q), dict(scr=lo + 8 * 499 // 256 * 256), dict(scr=up - need + 256), dict(scr=t, dlen=t + need - 8, lb=8)):
        rc, msg = call(sb=need, **kw)
        assert rc == ARG and b"scratch overlaps" in msg, kw
    assert np.array_equal(buf, before)


def test_no_needles_is_ok_after_the_checks_without_a_device(hiplib):
    """n_needles == 0 returns RDST_OK with no device work — with made-up pointers, so any device work would fault — but only
    after the argument checks"""
    buf, (k, q, lo, up, x, t) = _pointers()
    before = buf.copy()
    args = (k, 1000, None, 0, None, 0, lo, up, 8, x, BIG, 4, UNSIGNED, 4)
    assert _search(hiplib, *args) == OK
    assert _search(hiplib, *args, flags=1) == ARG
    assert _search(hiplib, k, 1000, None, 0, None, 0, None, None, 8, x, BIG, 4, UNSIGNED, 4) == ARG
    assert _search(hiplib, k, 1000, None, 0, None, 0, lo, up, 8, None, BIG, 4, UNSIGNED, 4) == ARG
    assert np.array_equal(buf, before)


def test_python_wrapper_refuses_host_operands_without_a_device():
    """the operand checks that need no device: what is not a HIP tensor is refused before the library is asked"""
    import torch
    import rdst_amd
    with pytest.raises(ValueError):
        rdst_amd.search_device_tensor(torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError):
        rdst_amd.unique_device_tensor(torch.zeros(8, dtype=torch.int32), inverse=True)


def test_cpp_source_compiles_and_links(tmp_path, hiplib):
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_search.cpp")
    exe = str(tmp_path / "test_rdst_search")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)


def test_host_half_under_sanitizers(tmp_path):
    """rdst_search.cpp with a main of its own, built with -fsanitize=address,undefined: a sanitizer report or a failed check
    is a non-zero exit.  Runs on the CPU as a child process; nothing is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "test_rdst_search_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_rdst_search_host.cpp"), os.path.join(CSRC, "rdst_search.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
