"""CPU-side checks of the segmented partial sort with device-resident offsets (rdst_hip_topk_segments_device_offsets,
..._scratch_bytes, rdst_hip_debug_topk_segments_plan_device): exported and declared in all three mirrors, every argument
error in the documented order, the no-ops, the scratch-size function, the source check behind "no wait, no copy", and the
host-only half under the sanitizers.  The pointers are made up: a call that got as far as the device would fault; the bytes
they point to are compared afterwards."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

import topk_segments_inputs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rdst_amd", "csrc")
OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
LARGEST = 1
NEW = ("rdst_hip_topk_segments_device_offsets", "rdst_hip_topk_segments_device_offsets_scratch_bytes", "rdst_hip_debug_topk_segments_plan_device")
WIDTHS = ((1, 0), (2, 0), (4, 0), (8, 0), (16, 0), (4, 4), (4, 8), (8, 4), (8, 8))
vp = ctypes.c_void_p
BIG = 1 << 40   # a scratch_bytes that is never too small


def _pointers():
    """five made-up 'device' pointers, 256-byte aligned, into one host buffer whose bytes are checked afterwards"""
    buf = np.random.default_rng(3).integers(0, 256, size=5 * 4096 + 256, dtype=np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    return buf, [base + 4096 * i for i in range(5)]


def _seg(lib, keys, n, off, ob, nseg, k, out, idx, ib, scratch, sbytes, far, kb, kind, levels, flags=0):
    return lib.rdst_hip_topk_segments_device_offsets(vp(keys), n, vp(off), ob, nseg, k, vp(out), vp(idx), ib, vp(scratch), sbytes, far, kb, kind, levels,
                                                     flags, None)


def test_symbols_header_and_mirrors(hiplib):
    import rdst_amd
    from rdst_amd import _lib
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(hiplib, name) is not None and name + "(" in header
    assert hiplib.rdst_hip_topk_segments_device_offsets.restype is ctypes.c_int and len(hiplib.rdst_hip_topk_segments_device_offsets.argtypes) == 17
    assert hiplib.rdst_hip_topk_segments_device_offsets_scratch_bytes.restype is ctypes.c_uint64
    assert len(hiplib.rdst_hip_debug_topk_segments_plan_device.argtypes) == 16
    assert "#define RDST_HIP_ABI_VERSION 2\n" in header and hiplib.rdst_hip_abi_version() == 2
    for name in ("topk_segments_device_offsets_tensor", "topk_segments_device_offsets_scratch_bytes", "topk_segments_plan_device"):
        assert name in rdst_amd.__all__ and callable(getattr(rdst_amd, name))
    hpp = open(os.path.join(ROOT, "include", "rdst.hpp")).read()
    assert hpp.count("void topk_segments_device_offsets(") == 2 and hpp.count("std::size_t topk_segments_device_offsets_scratch_bytes(") == 2
    assert "template <typename T, typename Off, typename Idx>\nvoid topk_segments_device_offsets(" in hpp
    from rdst_amd import build as B
    for unit in ("rdst_topk_segments_offsets.hip", "rdst_rank_args.cpp"):
        assert any(s.endswith(unit) for s in B.SOURCES)
    assert "fn rdst_hip_topk_segments_device_offsets(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the asynchrony, and the cliff, are stated where callers read them
    doc = " ".join(header.split("rdst_hip_topk_segments_device with the table of borders in DEVICE memory")[1].split("int rdst_hip_topk_segments_device_offsets(")[0]
                   .replace(" * ", " ").split())
    assert "no copy to or from the host, no wait on an event or on the stream, no staging buffer" in doc
    assert "THE STREAM CLASS HAS NO UPPER LENGTH" in doc and "performance cliff" in doc and "never a wrong answer" in doc


def _functions(code):
    """name -> body of every function defined at the top level of a translation unit (comments stripped)"""
    out = {}
    for m in re.finditer(r"^(?:extern \"C\" |template <[^\n]*>\n)?(?:__global__ [^\n]*? void|int|bool|PlanScratch|uint64_t) (\w+)\(", code, re.M):
        out[m.group(1)] = code[m.start():(code + "\n").index("\n}\n", m.start())]
    return out


def test_the_async_mode_reaches_no_wait_and_no_copy():
    """in the new translation unit the stream wait and the device-to-host copies stand in read_plan, read_far and the blocking
    test hook alone; only the wait mode calls the two readers, and the asynchronous path names none of the three"""
    code = "\n".join(line.split("//")[0] for line in open(os.path.join(CSRC, "rdst_topk_segments_offsets.hip")).read().splitlines())
    fns = _functions(code)
    for name in ("topk_segments_keygen_kernel", "topk_segments_items_kernel", "enqueue_plan_t", "enqueue_plan", "topk_segments_async", "read_plan", "read_far",
                 "topk_segments_wait", "rdst_hip_topk_segments_device_offsets", "rdst_hip_debug_topk_segments_plan_device"):
        assert name in fns, name
    blocking = ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipEventSynchronize", "hipStreamWaitEvent", "hipHostMalloc", "stage_segment_items",
                "sort_slice_locked")
    may_block = {"read_plan", "read_far", "rdst_hip_debug_topk_segments_plan_device"}
    for word in blocking:
        assert code.count(word) == sum(body.count(word) for body in fns.values()), word + " outside any function"
        for name, body in fns.items():
            assert word not in body or name in may_block, f"{word} in {name}"
    assert "hipStreamSynchronize" in fns["read_plan"] and "hipStreamSynchronize" in fns["read_far"]
    callers = {name for name, body in fns.items() if name not in may_block and ("read_plan(" in body or "read_far(" in body)}
    assert callers == {"topk_segments_wait"}
    assert [name for name, body in fns.items() if "topk_segments_wait(" in body and name != "topk_segments_wait"] == ["rdst_hip_topk_segments_device_offsets"]
    entry = fns["rdst_hip_topk_segments_device_offsets"]
    assert "if (async) return topk_segments_async(" in entry and entry.index("if (async) return topk_segments_async(") < entry.index("topk_segments_wait(")
    assert "const bool async = far_capacity == 0;" in entry
    for name in ("topk_segments_async", "enqueue_plan", "enqueue_plan_t"):
        for callee in ("read_plan", "read_far", "topk_segments_wait", "topk_slice_locked"):
            assert callee not in fns[name], f"{name} names {callee}"
    assert "rdst_internal::topk_segments_launch_locked(c, P.items, P.hdr, bounds)" in fns["topk_segments_async"]
    # the launches it reaches: rdst_topk_segments.hip, which the existing source check keeps free of waits and copies
    kernels = "\n".join(line.split("//")[0] for line in open(os.path.join(CSRC, "rdst_topk_segments.hip")).read().splitlines())
    hook = kernels.split("int rdst_internal::topk_segments_launch_locked(")[1].split("\n}\n")[0]
    assert "return launch_classes(c, items, hdr, counts);" in hook
    for word in blocking[:5]:
        assert word not in kernels, word
    for kernel in ("topk_segment_wave_counted_kernel", "topk_segment_block_counted_kernel", "topk_segment_stream_counted_kernel"):
        assert kernels.count(f"void {kernel}(") == 1
    for body in ("topk_segment_wave_body", "topk_segment_block_body", "topk_segment_stream_body"):
        assert kernels.count(f"void {body}(") == 1 and kernels.count(f"{body}<K, IDX>(") == 2      # one body, two kernels


def test_scratch_bytes_values_and_zeros(hiplib):
    f = hiplib.rdst_hip_topk_segments_device_offsets_scratch_bytes
    plan = hiplib.rdst_hip_sort_segments_device_offsets_scratch_bytes
    topk = hiplib.rdst_hip_topk_scratch_bytes
    for kb in (0, 3, 5, 32):
        assert f(10, 100, 5, kb, 0) == 0
    for kb in (1, 2, 16):
        assert f(10, 100, 5, kb, 4) == 0 and f(10, 100, 5, kb, 0) > 0
    assert f(10, 100, 5, 4, 3) == 0
    assert f(0, 100, 5, 4, 0) == 0 and f((1 << 30) + 1, 0, 5, 4, 0) == 0 and f(1 << 30, 0, 5, 4, 0) == plan(1 << 30) > 0
    assert f(10, 1 << 32, 5, 4, 0) == 0 and f(10, (1 << 64) - 1, 5, 4, 0) == 0 and f(10, (1 << 32) - 1, 5, 4, 0) > 0
    for kb, ib in WIDTHS:
        bm = S.block_max(kb, bool(ib))
        segs = (1, 2, 64, 65, 1000, 10**6, 1 << 30)
        fars = (0, 1, bm, bm + 1, 1 << 17, (1 << 17) + 1, 1 << 24, (1 << 32) - 1)
        ks = (1, 64, bm, bm + 1, 1 << 21, 1 << 40)
        cube = [[[int(f(n, far, k, kb, ib)) for k in ks] for far in fars] for n in segs]
        assert cube == [[[int(f(n, far, k, kb, ib)) for k in ks] for far in fars] for n in segs]                    # pure
        for i, n in enumerate(segs):
            assert plan(n) == 256 + 4 * ((4 * n + 255) // 256 * 256) + (16 * n + 255) // 256 * 256
            for j, far in enumerate(fars):
                for m, k in enumerate(ks):
                    assert cube[i][j][m] == plan(n) + (int(topk(far, min(k, far), kb, ib, 0)) if far else 0), (kb, ib, n, far, k)
                    if i: assert cube[i - 1][j][m] <= cube[i][j][m]                                                  # monotone in all three
                    if j: assert cube[i][j - 1][m] <= cube[i][j][m]
                    if m: assert cube[i][j][m - 1] <= cube[i][j][m]
    import rdst_amd
    assert rdst_amd.topk_segments_device_offsets_scratch_bytes(17, 0, 5, "uint32") == 1792
    assert rdst_amd.topk_segments_device_offsets_scratch_bytes(17, 1000, 5, "float64", 8) == 1792 + rdst_amd.topk_scratch_bytes(1000, 5, "float64", 8)


def test_key_argument_errors_are_the_host_offsets_entry_s(hiplib):
    """step 1, whatever the other arguments are: the code and message rdst_hip_topk_segments_device gives"""
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
        status = hiplib.rdst_hip_topk_segments_device(vp(keys), n, goodp, 2, 1, vp(o), None, 0, vp(s), BIG, kb, kind, levels, flags, None)
        assert status != OK
        msg = hiplib.rdst_hip_last_error()
        for off, ob, nseg, kk, out, idx, ib, scr, sb, far in ((t, 8, 2, 1, o, i, 4, s, BIG, 0), (None, 3, 3, 9, None, None, 0, None, 0, 1 << 40),
                                                              (t + 1, 4, 0, 0, o + 1, i + 1, 3, s + 1, 0, 7)):
            assert _seg(hiplib, keys, n, off, ob, nseg, kk, out, idx, ib, scr, sb, far, kb, kind, levels, flags) == status
            assert hiplib.rdst_hip_last_error() == msg
    assert np.array_equal(buf, before)


def test_argument_errors_in_their_order(hiplib):
    buf, (k, o, i, s, t) = _pointers()
    before = buf.copy()

    def call(keys=k, n=1000, off=t, ob=8, nseg=4, kk=10, out=o, idx=None, ib=0, scr=s, sb=BIG, far=0, kb=4, kind=UNSIGNED, flags=0):
        return _seg(hiplib, keys, n, off, ob, nseg, kk, out, idx, ib, scr, sb, far, kb, kind, kb, flags), hiplib.rdst_hip_last_error()

    # 1: len >= 2^32 before the flags; the flags before the no-ops
    assert call(n=1 << 32, flags=2, off=None, out=None, scr=None)[0] == UNSUPPORTED and b"2^32" in hiplib.rdst_hip_last_error()
    for kk, nseg in ((0, 4), (10, 0), (10, 4)):
        rc, msg = call(kk=kk, nseg=nseg, flags=2, off=None, out=None, scr=None)
        assert rc == ARG and b"flag" in msg
    # 2: k == 0 or no segment is a no-op: nothing else is looked at; no limit on k
    for flags in (0, LARGEST):
        for far in (0, 5, 1 << 40):
            assert call(kk=0, off=None, ob=3, out=None, idx=i + 1, ib=3, scr=None, sb=0, far=far, flags=flags)[0] == OK
            assert call(nseg=0, off=t + 1, ob=0, out=o + 1, idx=None, ib=99, scr=s + 1, sb=0, kb=16, far=far, flags=flags)[0] == OK
            assert call(kk=0, nseg=(1 << 30) + 1, out=None, scr=None, far=far, flags=flags)[0] == OK
    # 3: the table, before the outputs and the scratch — check_offsets_table's order and codes
    rc, msg = call(nseg=(1 << 30) + 1, ob=3, off=None, out=None, scr=None)
    assert rc == UNSUPPORTED and b"2^30" in msg
    assert call(nseg=1 << 30, out=None, scr=None)[0] == ARG and b"null key output" in hiplib.rdst_hip_last_error()
    for ob in (0, 1, 2, 3, 5, 16):
        rc, msg = call(ob=ob, off=None, out=None, scr=None)
        assert rc == ARG and b"offset_bytes" in msg
    rc, msg = call(off=None, out=None, scr=None, kk=1 << 40)
    assert rc == ARG and b"null offsets" in msg
    for ob, shift in ((4, 1), (4, 2), (8, 4), (8, 1)):
        rc, msg = call(off=t + shift, ob=ob, out=None, scr=None)
        assert rc == ALIGN and b"offsets pointer" in msg
    assert call(off=t + 4, ob=4, scr=None)[0] == ARG and b"null scratch" in hiplib.rdst_hip_last_error()
    # 4: the outputs, as the host-offsets entry checks them
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
    # 5: the scratch: NULL, alignment, far_capacity, size
    for far in (0, 1000, 1 << 32):
        rc, msg = call(scr=None, sb=0, far=far)
        assert rc == ARG and b"null scratch" in msg
        for shift in (1, 16, 128, 255):
            rc, msg = call(scr=s + shift, sb=0, far=far)
            assert rc == ALIGN and b"scratch not aligned" in msg
    for far in (1 << 32, (1 << 64) - 1):
        rc, msg = call(far=far)
        assert rc == ARG and b"far_capacity" in msg
    for kb, ib, kk, far in ((4, 0, 10, 0), (4, 4, 10, 1000), (8, 8, 1000, 1), (16, 0, 1, 0), (1, 0, 1 << 40, 1 << 20)):
        need = int(hiplib.rdst_hip_topk_segments_device_offsets_scratch_bytes(4, far, kk, kb, ib))
        assert need >= 256 + 4 * 256 + 256
        for sb in (0, 1, 256, need - 1):
            rc, msg = call(kk=kk, idx=i if ib else None, ib=ib, kb=kb, sb=sb, far=far)
            assert rc == ARG and b"rdst_hip_topk_segments_device_offsets_scratch_bytes" in msg, (kb, ib, kk, far, sb)
    assert np.array_equal(buf, before)


def test_plan_hook_argument_errors(hiplib):
    buf, (_k, _o, _i, s, t) = _pointers()
    before = buf.copy()
    counts = (ctypes.c_uint64 * 4)(9, 9, 9, 9)
    longest, flags = ctypes.c_uint64(9), ctypes.c_uint32(9)

    def hook(off=t, ob=8, nseg=4, n=1000, kk=5, kb=4, ib=0, unbounded=0, scr=s, sb=BIG, c=counts, lg=ctypes.byref(longest), fl=ctypes.byref(flags)):
        rc = hiplib.rdst_hip_debug_topk_segments_plan_device(vp(off), ob, nseg, n, kk, kb, ib, unbounded, vp(scr), sb, None, 0, c, lg, fl, None)
        return rc, hiplib.rdst_hip_last_error()

    assert hook(kb=3)[0] == UNSUPPORTED and hook(kb=2, ib=4)[0] == UNSUPPORTED and hook(ib=3)[0] == ARG
    assert hook(c=None)[0] == ARG and hook(lg=None)[0] == ARG and hook(fl=None)[0] == ARG
    for kwargs in ({"nseg": 0}, {"kk": 0}):
        counts[:] = (9, 9, 9, 9)
        longest.value, flags.value = 9, 9
        assert hook(off=None, scr=None, **kwargs)[0] == OK
        assert tuple(counts) == (0, 0, 0, 0) and longest.value == 0 and flags.value == 0
    assert hook(n=1 << 32)[0] == UNSUPPORTED
    assert hook(nseg=(1 << 30) + 1)[0] == UNSUPPORTED and hook(ob=2)[0] == ARG and hook(off=None)[0] == ARG and hook(off=t + 4)[0] == ALIGN
    assert hook(scr=None)[0] == ARG and hook(scr=s + 64)[0] == ALIGN
    need = int(hiplib.rdst_hip_topk_segments_device_offsets_scratch_bytes(4, 0, 5, 4, 0))
    rc, msg = hook(sb=need - 1)
    assert rc == ARG and b"scratch_bytes" in msg
    assert np.array_equal(buf, before)


def test_cpp_source_compiles_and_links(tmp_path, hiplib):
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_topk_segments_offsets.cpp")
    exe = str(tmp_path / "test_rdst_topk_segments_offsets")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)


def test_host_half_under_sanitizers(tmp_path):
    """rdst_rank_args.cpp and rdst_segments.cpp with a main of their own, built with -fsanitize=address,undefined:
    a sanitizer report or a failed check is a non-zero exit"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "test_rdst_topk_segments_offsets_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_rdst_topk_segments_offsets_host.cpp"), os.path.join(CSRC, "rdst_rank_args.cpp"),
           os.path.join(CSRC, "rdst_segments.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
