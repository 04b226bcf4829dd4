"""CPU-side checks of the runs of equal keys (rdst_hip_runs_device, rdst_hip_runs_scratch_bytes, rdst_hip_runs_limits): exported
and declared in all three mirrors, the arity, every argument error in the documented order with the sort's messages for the
key arguments, the scratch-size function, the source check behind "no wait, no copy", and the host-only half under the
sanitizers.  The pointers are made up: a call that got as far as the device would fault; the bytes they point to are compared
afterwards."""
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
PAD = 1
NEW = ("rdst_hip_runs_device", "rdst_hip_runs_scratch_bytes", "rdst_hip_runs_limits")
vp = ctypes.c_void_p
BIG = 1 << 40   # a scratch_bytes that is never too small


def _pointers():
    """six made-up 'device' pointers, 256-byte aligned and 8 KiB apart, into one host buffer whose bytes are checked afterwards"""
    buf = np.random.default_rng(5).integers(0, 256, size=6 * 8192 + 256, dtype=np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    return buf, [base + 8192 * i for i in range(6)]


def _runs(lib, keys, n, dlen, lb, out, starts, count, ob, cap, scratch, sbytes, kb, kind, levels, flags=0):
    return lib.rdst_hip_runs_device(vp(keys), n, vp(dlen), lb, vp(out), vp(starts), vp(count), ob, cap, vp(scratch), sbytes, kb, kind, levels, flags, None)


def test_symbols_header_and_mirrors(hiplib):
    import rdst_amd
    from rdst_amd import _lib
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(hiplib, name) is not None and name + "(" in header
    assert hiplib.rdst_hip_runs_device.restype is ctypes.c_int and len(hiplib.rdst_hip_runs_device.argtypes) == 16
    declared = header.split("int rdst_hip_runs_device(")[1].split(");")[0]
    assert declared.count(",") == 15                                              # the arity, as the header declares it
    assert hiplib.rdst_hip_runs_scratch_bytes.restype is ctypes.c_uint64 and len(hiplib.rdst_hip_runs_scratch_bytes.argtypes) == 2
    assert len(hiplib.rdst_hip_runs_limits.argtypes) == 2
    assert "#define RDST_RUNS_PAD_STARTS 1u\n" in header and _lib.RDST_RUNS_PAD_STARTS == 1
    assert "#define RDST_HIP_ABI_VERSION 2\n" in header and hiplib.rdst_hip_abi_version() == 2
    for name in ("runs_device_tensor", "runs_scratch_bytes", "runs_limits", "unique_device_tensor"):
        assert name in rdst_amd.__all__ and callable(getattr(rdst_amd, name))
    hpp = open(os.path.join(ROOT, "include", "rdst.hpp")).read()
    assert hpp.count("void runs_device(") == 1 and hpp.count("std::size_t runs_scratch_bytes(") == 1
    assert "template <typename T, typename Off, typename Len = std::uint64_t>\nvoid runs_device(" in hpp
    from rdst_amd import build as B
    for unit in ("rdst_runs.hip", "rdst_runs.cpp"):
        assert any(s.endswith(unit) for s in B.SOURCES)
    assert any(h.endswith("rdst_runs_layout.h") for h in B.HEADERS)
    assert "fn rdst_hip_runs_device(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    doc = " ".join(header.split("Runs of equal keys: the device twin")[1].split("int rdst_hip_runs_device(")[0].replace(" * ", " ").split())
    assert "no copy to or from the host, no wait on an event or on the stream, no library workspace" in doc
    assert "BIT-IDENTICAL" in doc and "THE ONLY DATA-DEPENDENT OUTCOMES are the two error bits" in doc and "A WRITE OF out_capacity OFFSETS" in doc


def _code(name):
    return "\n".join(line.split("//")[0] for line in open(os.path.join(CSRC, name)).read().splitlines())


def test_the_entry_reaches_no_wait_and_no_copy():
    """the two translation units name no synchronise, no copy (the only direction there is from here would be to or from the
    host), no event wait, no pinned memory and no hook that takes the library's workspace or sorts — the check the offsets
    entries have, over the whole of both files"""
    blocking = ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipEventSynchronize", "hipStreamWaitEvent", "hipEventRecord", "hipHostMalloc",
                "hipMalloc", "workspace_take", "stage_segment_items", "sort_slice", "HostJob")
    for unit in ("rdst_runs.hip", "rdst_runs.cpp"):
        code = _code(unit)
        for word in blocking:
            assert word not in code, f"{word} in {unit}"
    hip = _code("rdst_runs.hip")
    assert hip.count("__global__") == 2 and hip.count("rdst_internal::launch(") == 2 and hip.count("hipMemsetAsync(") == 1
    assert "hip" not in _code("rdst_runs.cpp").replace("rdst_hip", "").replace("rdst_kernels.hip", "").replace("rdst_runs.hip", "")
    # the shared helpers are the moved ones, defined once
    device_h, kernels = _code("rdst_device.h"), _code("rdst_kernels.hip")
    for text in ("S ld_relaxed(const S* p)", "void st_relaxed(S* p, S v)", "struct StatusWord", "constexpr uint32_t ST_EMPTY = 0, ST_AGG = 1, ST_INCL = 2;",
                 "constexpr uint32_t SPIN_LIMIT = 1u << 22;"):
        assert device_h.count(text) == 1 and text not in kernels and text not in hip, text
    assert "ld_relaxed<uint64_t>(status + idx)" in hip and "st_relaxed<uint64_t>(status + t" in hip and "SPIN_LIMIT" in hip


def test_scratch_bytes_and_limits(hiplib):
    import rdst_amd
    f = hiplib.rdst_hip_runs_scratch_bytes
    for kb in (0, 3, 5, 32):
        assert f(10, kb) == 0
    out = (ctypes.c_uint32 * 2)()
    assert hiplib.rdst_hip_runs_limits(4, None) == ARG and hiplib.rdst_hip_runs_limits(3, out) == UNSUPPORTED
    lens = (0, 1, 2, 4095, 4096, 4097, 16384, 16385, 10**6, 10**9, (1 << 32) - 1)
    for kb in (1, 2, 4, 8, 16):
        assert hiplib.rdst_hip_runs_limits(kb, out) == OK and tuple(out) == ({1: 16384, 2: 16384, 4: 8192, 8: 8192, 16: 4096}[kb], 8)
        assert f(1 << 32, kb) == 0 and f((1 << 64) - 1, kb) == 0
        got = [int(f(n, kb)) for n in lens]
        assert got == [int(f(n, kb)) for n in lens]                                 # pure
        assert got == sorted(got)                                                   # monotone in len
        assert got == [256 + (8 * max(1, -(-n // out[0])) + 255) // 256 * 256 for n in lens]
    assert rdst_amd.runs_scratch_bytes(10**6, "uint32") == 256 + 1024 and rdst_amd.runs_scratch_bytes(0, "u128") == 512


def test_key_argument_errors_are_the_sort_s(hiplib):
    """step 1, whatever the other arguments are: the code and message rdst_hip_sort_device gives"""
    buf, (k, o, s, c, x, t) = _pointers()
    before = buf.copy()
    calls = [(k, 8, 3, UNSIGNED, 3), (k, 8, 0, UNSIGNED, 0), (k, 8, 32, UNSIGNED, 32), (k, 8, 2, FLOAT, 2), (k, 8, 16, FLOAT, 16), (k, 8, 4, UNSIGNED, 0),
             (k, 8, 4, SIGNED, 3), (k, 8, 8, SIGNED, 4), (k, 8, 1, UNSIGNED, 2), (k, 8, 4, BYTES_BE, 4), (k, 8, 16, BYTES_BE, 16), (k, 8, 4, 4, 4),
             (k, 8, 4, -1, 4), (None, 8, 4, UNSIGNED, 4), (None, 1, 4, UNSIGNED, 4), (k + 2, 8, 4, UNSIGNED, 4), (k + 8, 8, 16, UNSIGNED, 16),
             (k + 1, 1, 2, SIGNED, 2), (k, 1 << 36, 4, UNSIGNED, 4)]
    for keys, n, kb, kind, levels in calls:
        status = hiplib.rdst_hip_sort_device(vp(keys), vp(t), n, kb, kind, levels, None)
        assert status != OK
        msg = hiplib.rdst_hip_last_error()
        for dlen, lb, out, starts, count, ob, cap, scr, sb, flags in ((None, 0, o, s, c, 8, 8, x, BIG, 0), (k + 1, 3, k, k, None, 3, 8, None, 0, 6),
                                                                      (None, 0, None, None, c, 4, 0, x + 1, 0, PAD)):
            assert _runs(hiplib, keys, n, dlen, lb, out, starts, count, ob, cap, scr, sb, kb, kind, levels, flags) == status
            assert hiplib.rdst_hip_last_error() == msg
    assert np.array_equal(buf, before)


def test_argument_errors_in_their_order(hiplib):
    buf, (k, o, s, c, x, t) = _pointers()
    before = buf.copy()

    def call(keys=k, n=1000, dlen=None, lb=0, out=o, starts=s, count=c, ob=8, cap=500, scr=x, sb=BIG, kb=4, kind=UNSIGNED, flags=0):
        return _runs(hiplib, keys, n, dlen, lb, out, starts, count, ob, cap, scr, sb, kb, kind, kb, flags), hiplib.rdst_hip_last_error()

    bad = dict(dlen=t + 1, lb=3, ob=3, count=None, out=k, scr=None)              # everything behind the step under test is wrong too
    # 3: len >= 2^32 before the flags; 4: the flags before the length
    rc, msg = call(n=1 << 32, flags=2, **bad)
    assert rc == UNSUPPORTED and b"2^32" in msg
    for flags in (2, 3, 0x80000000):
        rc, msg = call(flags=flags, **bad)
        assert rc == ARG and b"flag" in msg
    # 5: the device-resident length, only when there is one
    for lb in (0, 1, 2, 3, 5, 16):
        rc, msg = call(**dict(bad, lb=lb))
        assert rc == ARG and b"device-resident length" in msg
    for lb, shift in ((4, 1), (4, 2), (8, 4), (8, 1)):
        rc, msg = call(**dict(bad, dlen=t + shift, lb=lb))
        assert rc == ALIGN and b"length pointer" in msg
    # 6: offset_bytes (without dev_len, len_bytes is not looked at)
    for ob in (0, 1, 2, 3, 5, 16):
        rc, msg = call(**dict(bad, dlen=None, lb=99, ob=ob))
        assert rc == ARG and b"offset_bytes" in msg
    # 7: the run count
    rc, msg = call(**dict(bad, dlen=t, lb=4, ob=4))
    assert rc == ARG and b"null run count" in msg
    for ob, shift in ((4, 1), (4, 2), (8, 4), (8, 1)):
        rc, msg = call(count=c + shift, ob=ob, out=k, scr=None)
        assert rc == ALIGN and b"run count pointer" in msg
    rc, msg = call(count=k + 4 * 999, ob=4, out=k, scr=None)
    assert rc == ARG and b"run count overlaps the input" in msg
    # 8: the outputs, with a capacity: alignment, then overlap, then PAD without starts; each may be NULL
    for kb, shift in ((2, 1), (4, 2), (8, 4), (16, 8)):
        rc, msg = call(out=o + shift, kb=kb, starts=s + 1, scr=None, n=100, cap=50)
        assert rc == ALIGN and b"key output" in msg
    for ob, shift in ((4, 1), (4, 2), (8, 4), (8, 1)):
        rc, msg = call(starts=s + shift, ob=ob, out=k, scr=None)
        assert rc == ALIGN and b"starts output" in msg
    for kw in (dict(out=k), dict(out=k + 4 * 999), dict(out=k - 4 * 499), dict(starts=k), dict(starts=k - 8 * 500), dict(starts=k + 4 * 999 - 3996 % 8)):
        rc, msg = call(scr=None, flags=PAD, **kw)
        assert rc == ARG and b"overlaps the input" in msg, kw
    for kw in (dict(starts=o), dict(starts=o + 4 * 499 - 4), dict(count=o), dict(count=s + 8 * 500), dict(out=s + 8 * 500)):
        rc, msg = call(scr=None, flags=PAD, **kw)
        assert rc == ARG and b"overlap each other" in msg, kw
    for kw in (dict(out=k - 4 * 500), dict(out=k + 4 * 1000), dict(starts=k - 8 * 501), dict(count=s + 8 * 501), dict(starts=o + 4 * 500)):   # touching is no overlap
        rc, msg = call(scr=None, **kw)
        assert rc == ARG and b"null scratch" in msg, kw
    rc, msg = call(starts=None, flags=PAD, scr=None)
    assert rc == ARG and b"RDST_RUNS_PAD_STARTS" in msg
    for kw in (dict(out=None), dict(starts=None), dict(out=None, starts=None)):
        rc, msg = call(scr=None, **kw)
        assert rc == ARG and b"null scratch" in msg
    # capacity 0: the output pointers are not looked at, PAD included
    rc, msg = call(cap=0, out=k + 1, starts=k + 3, flags=PAD, scr=None)
    assert rc == ARG and b"null scratch" in msg
    # 9: the scratch
    for shift in (1, 16, 128, 255):
        rc, msg = call(scr=x + shift, sb=0)
        assert rc == ALIGN and b"scratch not aligned" in msg
    for kb, n in ((4, 1000), (1, 0), (16, 10**6), (8, (1 << 32) - 1)):
        need = int(hiplib.rdst_hip_runs_scratch_bytes(n, kb))
        assert need >= 512
        for sb in (0, 1, 256, need - 1):
            rc, msg = call(n=n, kb=kb, sb=sb, cap=0, keys=k if n else None, count=k - 64)          # (in front of the longest input)
            assert rc == ARG and b"rdst_hip_runs_scratch_bytes" in msg, (kb, n, sb)
    assert np.array_equal(buf, before)


def test_python_wrapper_refuses_host_operands_without_a_device():
    """the operand checks that need no device: what is not a HIP tensor is refused before the library is asked"""
    import torch
    import rdst_amd
    with pytest.raises(ValueError):
        rdst_amd.runs_device_tensor(torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError):
        rdst_amd.unique_device_tensor(torch.zeros(8, dtype=torch.int32))


def test_cpp_source_compiles_and_links(tmp_path, hiplib):
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_runs.cpp")
    exe = str(tmp_path / "test_rdst_runs")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)


def test_host_half_under_sanitizers(tmp_path):
    """rdst_runs.cpp with a main of its own, built with -fsanitize=address,undefined: a sanitizer report or a failed check is a
    non-zero exit.  Runs on the CPU as a child process; nothing is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "test_rdst_runs_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_rdst_runs_host.cpp"), os.path.join(CSRC, "rdst_runs.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
