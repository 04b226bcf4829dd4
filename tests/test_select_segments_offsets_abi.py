"""CPU-side checks of the segmented select with device-resident offsets (rdst_hip_select_segments_device_offsets,
..._scratch_bytes): exported and declared in all three mirrors, every argument error in the documented order, the no-ops, the
scratch-size function, the source check behind "no wait, no copy", and the host-only half under the sanitizers.  The pointers
are made up: a call that got as far as the device would fault; the bytes they point to are compared afterwards."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import select_segments_inputs as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rdst_amd", "csrc")
OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
LARGEST = 1
NEW = ("rdst_hip_select_segments_device_offsets", "rdst_hip_select_segments_device_offsets_scratch_bytes")
WIDTHS = ((1, 0), (2, 0), (4, 0), (8, 0), (16, 0), (4, 4), (4, 8), (8, 4), (8, 8))
GOOD = [(0, 0, 0), (1, 2, 0), (9, 10, 2)]
vp = ctypes.c_void_p
BIG = 1 << 40   # a scratch_bytes that is never too small


def _pointers():
    """five made-up 'device' pointers, 256-byte aligned, into one host buffer whose bytes are checked afterwards"""
    buf = np.random.default_rng(3).integers(0, 256, size=5 * 4096 + 256, dtype=np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    return buf, [base + 4096 * i for i in range(5)]


def _specs(specs):
    from rdst_amd import _lib
    if specs is None:
        return None
    return (_lib.RankSpecC * max(len(specs), 1))(*(_lib.RankSpecC(*(tuple(s) + (0,))[:4]) for s in specs))


def _seg(lib, keys, n, off, ob, nseg, specs, nr, out, idx, ib, scratch, sbytes, far, kb, kind, levels, flags=0):
    return lib.rdst_hip_select_segments_device_offsets(vp(keys), n, vp(off), ob, nseg, _specs(specs), nr, vp(out), vp(idx), ib, vp(scratch), sbytes, far, kb,
                                                       kind, levels, flags, None)


def test_symbols_header_and_mirrors(hiplib):
    import rdst_amd
    from rdst_amd import _lib
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(hiplib, name) is not None and name + "(" in header
    assert hiplib.rdst_hip_select_segments_device_offsets.restype is ctypes.c_int and len(hiplib.rdst_hip_select_segments_device_offsets.argtypes) == 18
    assert hiplib.rdst_hip_select_segments_device_offsets_scratch_bytes.restype is ctypes.c_uint64
    assert "#define RDST_HIP_ABI_VERSION 2\n" in header and hiplib.rdst_hip_abi_version() == 2
    for name in ("select_segments_device_offsets_tensor", "select_segments_device_offsets_scratch_bytes"):
        assert name in rdst_amd.__all__ and callable(getattr(rdst_amd, name))
    hpp = open(os.path.join(ROOT, "include", "rdst.hpp")).read()
    assert hpp.count("void select_segments_device_offsets(") == 2 and hpp.count("std::size_t select_segments_device_offsets_scratch_bytes(") == 2
    assert "template <typename T, typename Off, typename Idx>\nvoid select_segments_device_offsets(" in hpp
    from rdst_amd import build as B
    for unit in ("rdst_select_segments_offsets.hip", "rdst_rank_args.cpp"):
        assert any(s.endswith(unit) for s in B.SOURCES)
    assert "fn rdst_hip_select_segments_device_offsets(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the asynchrony, the cliff and the plan hook are stated where callers read them
    doc = " ".join(header.split("rdst_hip_select_segments_device with the table of borders in DEVICE memory")[1]
                   .split("int rdst_hip_select_segments_device_offsets(")[0].replace(" * ", " ").split())
    assert "no copy to or from the host, no wait on an event or on the stream, no staging buffer" in doc
    assert "THE STREAM CLASS HAS NO UPPER LENGTH" in doc and "performance cliff" in doc and "never a wrong answer" in doc
    assert "NO DATA-DEPENDENT FAILURE except an invalid table" in doc
    assert "rdst_hip_debug_topk_segments_plan_device with k = 1" in doc


def _functions(code):
    """name -> body of every function defined at the top level of a translation unit (comments stripped)"""
    out = {}
    for m in re.finditer(r"^(?:extern \"C\" |template <[^\n]*>\n)?(?:__global__ [^\n]*? void|__device__ [^\n]*? void|int|bool|uint64_t) ((?:\w+::)?\w+)\(", code, re.M):
        out[m.group(1)] = code[m.start():(code + "\n").index("\n}\n", m.start())]
    return out


def _code(name):
    return "\n".join(line.split("//")[0] for line in open(os.path.join(CSRC, name)).read().splitlines())


def test_the_async_mode_reaches_no_wait_and_no_copy():
    """in the new translation unit the stream wait and the device-to-host copies stand in read_header and read_far_items alone;
    only the wait mode calls the two readers, and the asynchronous path and the launch hook name none of them"""
    code = _code("rdst_select_segments_offsets.hip")
    fns = _functions(code)
    for name in ("select_segments_async", "read_header", "read_far_items", "run_far_segments", "select_segments_wait", "rdst_hip_select_segments_device_offsets"):
        assert name in fns, name
    blocking = ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipEventSynchronize", "hipStreamWaitEvent", "hipHostMalloc", "stage_segment_items",
                "sort_slice_locked")
    may_block = {"read_header", "read_far_items"}
    for word in blocking:
        assert code.count(word) == sum(body.count(word) for body in fns.values()), word + " outside any function"
        for name, body in fns.items():
            assert word not in body or name in may_block, f"{word} in {name}"
    assert "hipStreamSynchronize" in fns["read_header"] and "hipStreamSynchronize" in fns["read_far_items"]
    callers = {name for name, body in fns.items() if name not in may_block and ("read_header(" in body or "read_far_items(" in body)}
    assert callers == {"select_segments_wait"}
    assert [name for name, body in fns.items() if "select_segments_wait(" in body and name != "select_segments_wait"] == ["rdst_hip_select_segments_device_offsets"]
    entry = fns["rdst_hip_select_segments_device_offsets"]
    assert "if (async) return select_segments_async(" in entry and entry.index("if (async) return select_segments_async(") < entry.index("select_segments_wait(")
    assert "const bool async = far_capacity == 0;" in entry
    for callee in ("read_header", "read_far_items", "select_segments_wait", "run_far_segments", "select_slice_locked", "resolve("):
        assert callee not in fns["select_segments_async"], f"select_segments_async names {callee}"
    assert "rdst_internal::select_segments_launch_locked(c, P.items, P.hdr, bounds, ranks)" in fns["select_segments_async"]
    assert "rdst_internal::topk_segments_plan_locked(" in fns["select_segments_async"]
    # the plan it reaches: the hook of rdst_topk_segments_offsets.hip, which enqueues and names no reader; the plan kernels exist once
    plan = _code("rdst_topk_segments_offsets.hip")
    hook = plan.split("int rdst_internal::topk_segments_plan_locked(")[1].split("\n}\n")[0]
    assert "return enqueue_plan(" in hook
    for word in blocking + ("read_plan", "read_far", "topk_segments_wait"):
        assert word not in hook, word
    assert "_kernel" not in code.replace("select_segment_", "") and "__global__" not in code
    # the launches it reaches: rdst_select_segments.hip, free of waits and copies; one body, two kernels
    kernels = _code("rdst_select_segments.hip")
    hook = kernels.split("int rdst_internal::select_segments_launch_locked(")[1].split("\n}\n")[0]
    assert "launch_round(c, items, hdr, counts, rs)" in hook
    for word in blocking[:5]:
        assert word not in kernels, word
    for kernel in ("select_segment_wave_kernel", "select_segment_block_kernel", "select_segment_stream_kernel", "select_segment_wave_counted_kernel",
                   "select_segment_block_counted_kernel", "select_segment_stream_counted_kernel"):
        assert kernels.count(f"void {kernel}(") == 1
    for body in ("select_segment_wave_body", "select_segment_block_body", "select_segment_stream_body"):
        assert kernels.count(f"void {body}(") == 1 and kernels.count(f"{body}<K, IDX>(") == 2      # one body, two kernels
    for counted in ("wave", "block", "stream"):
        assert f"HDR_TOPK_RUN_{counted.upper()}" in _functions(kernels)[f"select_segment_{counted}_counted_kernel"]


def test_scratch_bytes_values_and_zeros(hiplib):
    f = hiplib.rdst_hip_select_segments_device_offsets_scratch_bytes
    plan = hiplib.rdst_hip_sort_segments_device_offsets_scratch_bytes
    select = hiplib.rdst_hip_select_scratch_bytes
    for kb in (0, 3, 5, 32):
        assert f(10, 100, 5, kb, 0) == 0
    for kb in (1, 2, 16):
        assert f(10, 100, 5, kb, 4) == 0 and f(10, 100, 5, kb, 0) > 0
    assert f(10, 100, 5, 4, 3) == 0
    assert f(0, 100, 5, 4, 0) == 0 and f((1 << 30) + 1, 0, 5, 4, 0) == 0 and f(1 << 30, 0, 5, 4, 0) == plan(1 << 30) > 0
    assert f(10, 1 << 32, 5, 4, 0) == 0 and f(10, (1 << 64) - 1, 5, 4, 0) == 0 and f(10, (1 << 32) - 1, 5, 4, 0) > 0
    for kb, ib in WIDTHS:
        _wm, bm, sm, _mr = Q.limits(kb, bool(ib))
        segs = (1, 2, 64, 65, 1000, 10**6, 1 << 30)
        fars = (0, 1, bm, bm + 1, sm, sm + 1, 1 << 24, (1 << 32) - 1)
        nrs = (1, 32, 33, 70, 1 << 20)
        cube = [[[int(f(n, far, nr, kb, ib)) for nr in nrs] for far in fars] for n in segs]
        assert cube == [[[int(f(n, far, nr, kb, ib)) for nr in nrs] for far in fars] for n in segs]                 # pure
        for i, n in enumerate(segs):
            assert plan(n) == 256 + 4 * ((4 * n + 255) // 256 * 256) + (16 * n + 255) // 256 * 256
            for j, far in enumerate(fars):
                for m, nr in enumerate(nrs):
                    assert cube[i][j][m] == plan(n) + (int(select(far, nr, kb, ib, 0)) if far else 0), (kb, ib, n, far, nr)
                    if i: assert cube[i - 1][j][m] <= cube[i][j][m]                                                  # monotone in all three
                    if j: assert cube[i][j - 1][m] <= cube[i][j][m]
                    if m: assert cube[i][j][m - 1] <= cube[i][j][m]
    import rdst_amd
    assert rdst_amd.select_segments_device_offsets_scratch_bytes(17, 0, 5, "uint32") == 1792
    assert rdst_amd.select_segments_device_offsets_scratch_bytes(17, 1000, 5, "float64", 8) == 1792 + rdst_amd.select_scratch_bytes(1000, 5, "float64", 8)


def test_key_argument_errors_are_the_host_offsets_entry_s(hiplib):
    """step 1, whatever the other arguments are: the code and message rdst_hip_select_segments_device gives"""
    buf, (k, o, i, s, t) = _pointers()
    before = buf.copy()
    good = np.array([0, 4, 8], dtype=np.uint64)
    goodp = good.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    calls = [
        (k, 8, 3, UNSIGNED, 3, 0), (k, 8, 0, UNSIGNED, 0, 0), (k, 8, 32, UNSIGNED, 32, 0), (k, 8, 2, FLOAT, 2, 0), (k, 8, 16, FLOAT, 16, 0),
        (k, 8, 4, UNSIGNED, 0, 0), (k, 8, 4, SIGNED, 3, 0), (k, 8, 8, SIGNED, 4, 0), (k, 8, 1, UNSIGNED, 2, 0),
        (k, 8, 4, BYTES_BE, 4, 0), (k, 8, 16, BYTES_BE, 16, 0), (k, 8, 4, 4, 4, 0), (k, 8, 4, -1, 4, 0),
        (None, 8, 4, UNSIGNED, 4, 0), (None, 1, 4, UNSIGNED, 4, 0),
        (k + 2, 8, 4, UNSIGNED, 4, 0), (k + 8, 8, 16, UNSIGNED, 16, 0), (k + 1, 1, 2, SIGNED, 2, 0),
        (k, 1 << 32, 4, UNSIGNED, 4, 0), (k, (1 << 36) - 1, 8, FLOAT, 8, LARGEST),
        (k, 8, 4, UNSIGNED, 4, 2), (k, 8, 4, UNSIGNED, 4, 3), (k, 8, 4, UNSIGNED, 4, 0x80000000),
    ]
    for keys, n, kb, kind, levels, flags in calls:
        status = hiplib.rdst_hip_select_segments_device(vp(keys), n, goodp, 2, _specs(GOOD), 3, vp(o), None, 0, vp(s), BIG, kb, kind, levels, flags, None)
        assert status != OK
        msg = hiplib.rdst_hip_last_error()
        for off, ob, nseg, specs, nr, out, idx, ib, scr, sb, far in ((t, 8, 2, GOOD, 3, o, i, 4, s, BIG, 0), (None, 3, 3, None, 9, None, None, 0, None, 0, 1 << 40),
                                                                     (t + 1, 4, 0, [(3, 2, 0)], 0, o + 1, i + 1, 3, s + 1, 0, 7)):
            assert _seg(hiplib, keys, n, off, ob, nseg, specs, nr, out, idx, ib, scr, sb, far, kb, kind, levels, flags) == status
            assert hiplib.rdst_hip_last_error() == msg
    assert np.array_equal(buf, before)


def test_argument_errors_in_their_order(hiplib):
    buf, (k, o, i, s, t) = _pointers()
    before = buf.copy()
    unset = object()

    def call(keys=k, n=1000, off=t, ob=8, nseg=4, specs=GOOD, nr=unset, out=o, idx=None, ib=0, scr=s, sb=BIG, far=0, kb=4, kind=UNSIGNED, flags=0):
        nr = (len(specs) if specs is not None else 0) if nr is unset else nr
        return _seg(hiplib, keys, n, off, ob, nseg, specs, nr, out, idx, ib, scr, sb, far, kb, kind, kb, flags), hiplib.rdst_hip_last_error()

    # 1: len >= 2^32 before the flags; the flags before the no-ops
    assert call(n=1 << 32, flags=2, off=None, specs=None, nr=2, out=None, scr=None)[0] == UNSUPPORTED and b"2^32" in hiplib.rdst_hip_last_error()
    for nr, nseg in ((0, 4), (3, 0), (3, 4)):
        rc, msg = call(nr=nr, nseg=nseg, flags=2, off=None, specs=None, out=None, scr=None)
        assert rc == ARG and b"flag" in msg
    # 2: no rank or no segment is a no-op: nothing else is looked at
    for flags in (0, LARGEST):
        for far in (0, 5, 1 << 40):
            assert call(nr=0, off=None, ob=3, specs=None, out=None, idx=i + 1, ib=3, scr=None, sb=0, far=far, flags=flags)[0] == OK
            assert call(nseg=0, off=t + 1, ob=0, specs=[(3, 2, 0)], out=o + 1, idx=None, ib=99, scr=s + 1, sb=0, kb=16, far=far, flags=flags)[0] == OK
            assert call(nr=0, nseg=(1 << 30) + 1, out=None, scr=None, far=far, flags=flags)[0] == OK
    # 3: the table, before the ranks, the outputs and the scratch — check_offsets_table's order and codes
    rc, msg = call(nseg=(1 << 30) + 1, ob=3, off=None, specs=None, nr=2, out=None, scr=None)
    assert rc == UNSUPPORTED and b"2^30" in msg
    assert call(nseg=1 << 30, out=None, scr=None)[0] == ARG and b"null key output" in hiplib.rdst_hip_last_error()
    for ob in (0, 1, 2, 3, 5, 16):
        rc, msg = call(ob=ob, off=None, specs=None, nr=2, out=None, scr=None)
        assert rc == ARG and b"offset_bytes" in msg
    rc, msg = call(off=None, specs=[(3, 2, 0)], out=None, scr=None)
    assert rc == ARG and b"null offsets" in msg
    for ob, shift in ((4, 1), (4, 2), (8, 4), (8, 1)):
        rc, msg = call(off=t + shift, ob=ob, specs=None, nr=1, out=None, scr=None)
        assert rc == ALIGN and b"offsets pointer" in msg
    assert call(off=t + 4, ob=4, scr=None)[0] == ARG and b"null scratch" in hiplib.rdst_hip_last_error()
    # 4: NULL ranks, then a bad spec; the message names the first
    rc, msg = call(specs=None, nr=3, out=None, scr=None)
    assert rc == ARG and b"null ranks" in msg
    bad = {"num > den": (3, 2, 0), "mode": (1, 2, 3), "reserved": (1, 2, 0, 1), "absolute with a mode": (5, 0, 1)}
    for what, spec in bad.items():
        for at in (0, 2, 40):
            specs = [(1, 2, 0)] * at + [spec, (7, 3, 9)]
            rc, msg = call(specs=specs, out=None, idx=i + 1, ib=3, scr=None)
            assert rc == ARG and f"ranks[{at}]".encode() in msg, (what, msg)
    # absolute ranks past every segment, repeats, any order: no error
    assert call(specs=[((1 << 32) - 1, 0, 0), (0, 0, 0), (0, 0, 0), (1, 1, 2)], scr=None)[0] == ARG and b"null scratch" in hiplib.rdst_hip_last_error()
    # 5: the outputs, as the host-offsets entry checks them
    rc, msg = call(out=None, idx=i, ib=3, scr=None)
    assert rc == ARG and b"null key output" in msg
    for kb, shift in ((2, 1), (4, 2), (8, 4), (16, 8)):
        rc, msg = call(out=o + shift, kb=kb, idx=i, ib=3, scr=None)
        assert rc == ALIGN and b"key output" in msg
    for ib in (0, 1, 2, 3, 5, 16):
        rc, msg = call(idx=i + 1, ib=ib, kb=2, kind=SIGNED, scr=None)
        assert rc == ARG and b"index_bytes" in msg
    for kb in (1, 2, 16):
        for ib in (4, 8):
            rc, msg = call(idx=i + 1, ib=ib, kb=kb, scr=None)
            assert rc == UNSUPPORTED and b"4- or 8-byte keys" in msg
    for ib, shift in ((4, 1), (4, 2), (8, 4), (8, 1)):
        rc, msg = call(idx=i + shift, ib=ib, kb=8, kind=FLOAT, scr=None)
        assert rc == ALIGN and b"index output" in msg
    for ib in (0, 3, 99):                                                   # without an index, index_bytes is not looked at
        assert call(idx=None, ib=ib, scr=None)[0] == ARG and b"null scratch" in hiplib.rdst_hip_last_error()
    # 6: the scratch: NULL, alignment, far_capacity, size
    for far in (0, 1000, 1 << 32):
        rc, msg = call(scr=None, sb=0, far=far)
        assert rc == ARG and b"null scratch" in msg
        for shift in (1, 16, 128, 255):
            rc, msg = call(scr=s + shift, sb=0, far=far)
            assert rc == ALIGN and b"scratch not aligned" in msg
    for far in (1 << 32, (1 << 64) - 1):
        rc, msg = call(far=far)
        assert rc == ARG and b"far_capacity" in msg
    for kb, ib, far in ((4, 0, 0), (4, 4, 1000), (8, 8, 1), (16, 0, 0), (1, 0, 1 << 20)):
        need = int(hiplib.rdst_hip_select_segments_device_offsets_scratch_bytes(4, far, 3, kb, ib))
        assert need >= 256 + 4 * 256 + 256
        for sb in (0, 1, 256, need - 1):
            rc, msg = call(idx=i if ib else None, ib=ib, kb=kb, sb=sb, far=far)
            assert rc == ARG and b"rdst_hip_select_segments_device_offsets_scratch_bytes" in msg, (kb, ib, far, sb)
    assert np.array_equal(buf, before)


def test_python_wrapper_refuses_host_operands_without_a_device():
    """the operand checks that need no device: what is not a HIP tensor is refused before the library is asked"""
    import torch
    import rdst_amd
    with pytest.raises(ValueError):
        rdst_amd.select_segments_device_offsets_tensor(torch.zeros(8, dtype=torch.int32), torch.tensor([0, 8]), ranks=[0])


def test_cpp_source_compiles_and_links(tmp_path, hiplib):
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_select_segments_offsets.cpp")
    exe = str(tmp_path / "test_rdst_select_segments_offsets")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)


def test_host_half_under_sanitizers(tmp_path):
    """rdst_rank_args.cpp and rdst_segments.cpp with a main of their own, built with -fsanitize=address,undefined:
    a sanitizer report or a failed check is a non-zero exit.  Runs on the CPU; nothing is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "test_rdst_select_segments_offsets_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_rdst_select_segments_offsets_host.cpp"), os.path.join(CSRC, "rdst_rank_args.cpp"),
           os.path.join(CSRC, "rdst_segments.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
