"""CPU-side checks of the segmented select's entries (rdst_hip_select_segments_device, ..._scratch_bytes, ..._limits,
rdst_rank_for_length): exported and declared in all three mirrors, every argument error in the documented order — the shared
arguments with rdst_hip_topk_segments_device's codes —, the no-ops, and the two pure functions.  The pointers are made up: a
call that got as far as the device would fault; the bytes they point to are compared afterwards."""
import ctypes
import os

import numpy as np
import pytest

import select_segments_inputs as Q
import topk_segments_inputs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED, ALIGN = 0, -1, -2, -6
UNSIGNED, SIGNED, FLOAT, BYTES_BE = 0, 1, 2, 3
LARGEST = 1
NEW = ("rdst_hip_select_segments_device", "rdst_hip_select_segments_scratch_bytes", "rdst_hip_select_segments_limits", "rdst_rank_for_length")
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


def _specs(specs):
    from rdst_amd import _lib
    if specs is None:
        return None
    return (_lib.RankSpecC * max(len(specs), 1))(*(_lib.RankSpecC(*(tuple(s) + (0,))[:4]) for s in specs))


GOOD = [(0, 0, 0), (1, 2, 0), (9, 10, 2)]


@pytest.fixture
def setter(hiplib):
    yield hiplib.rdst_hip_set_topk_segments_stream_max
    hiplib.rdst_hip_set_topk_segments_stream_max(0)


def _seg(lib, keys, n, off, nseg, specs, nr, out, idx, ib, scratch, sbytes, kb, kind, levels, flags=0):
    return lib.rdst_hip_select_segments_device(vp(keys), n, off, nseg, _specs(specs), nr, vp(out), vp(idx), ib, vp(scratch), sbytes, kb, kind, levels,
                                               flags, None)


def test_symbols_header_and_mirrors(hiplib):
    import rdst_amd
    from rdst_amd import _lib
    header = open(os.path.join(ROOT, "include", "rdst_hip.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(hiplib, name) is not None and name + "(" in header
    assert hiplib.rdst_hip_select_segments_device.restype is ctypes.c_int and len(hiplib.rdst_hip_select_segments_device.argtypes) == 16
    assert hiplib.rdst_hip_select_segments_scratch_bytes.restype is ctypes.c_uint64
    assert ctypes.sizeof(_lib.RankSpecC) == 16 and "typedef struct { uint32_t num, den, mode, reserved; } rdst_rank_spec;" in header
    for name, value in (("RDST_RANK_LOWER", 0), ("RDST_RANK_HIGHER", 1), ("RDST_RANK_NEAREST", 2)):
        assert f"#define {name} " in header and getattr(_lib, name) == value
    assert "#define RDST_HIP_ABI_VERSION 2\n" in header and hiplib.rdst_hip_abi_version() == 2
    for name in ("select_segments_device_tensor", "select_rows_tensor", "select_segments_scratch_bytes", "select_segments_limits", "rank_for_length"):
        assert name in rdst_amd.__all__ and callable(getattr(rdst_amd, name))
    hpp = open(os.path.join(ROOT, "include", "rdst.hpp")).read()
    assert hpp.count("void select_segments(") == 2 and "template <typename T, typename Idx>\nvoid select_segments(" in hpp
    from rdst_amd import build as B
    assert any(s.endswith("rdst_select_segments.hip") for s in B.SOURCES)
    for h in ("rdst_segments_device.h", "rdst_rank_rule.h"):
        assert any(p.endswith(h) for p in B.HEADERS)


def test_one_rank_rule_and_shared_device_code():
    """the rule is stated once, for the host and the kernels; what the two segmented files share lives in one header, and the far
    class runs on the select's hook, which never waits"""
    csrc = os.path.join(ROOT, "rdst_amd", "csrc")

    def code(name):
        return "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, name)).read().splitlines())

    rule, seg, sel, topk, shared = (code(n) for n in ("rdst_rank_rule.h", "rdst_segments.cpp", "rdst_select_segments.hip", "rdst_topk_segments.hip",
                                                     "rdst_segments_device.h"))
    assert "float" not in rule and "double" not in rule and rule.count("bool resolve(") == 1
    assert "rdst_rank_rule::resolve(" in seg and sel.count("rdst_rank_rule::resolve(") == 2     # the kernels' step, and the far class on the host
    assert "hip_runtime" not in seg
    for name in ("void block_order(", "struct BlockLds", "void wave_order(", "void collect_trip(", "KeyVec<K> load_vec(", "void count_digits("):
        assert shared.count(name) == 1 and name not in sel and name not in topk, name
    assert "rdst_internal::select_slice_locked(" in sel and "rdst_internal::stage_segment_items(" in sel
    for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipEventSynchronize", "sort_slice_locked"):
        assert word not in sel, word
    select = code("rdst_select.hip")
    assert select.count("rdst_internal::select_slice_locked(") == 2                             # defined once, called by the entry


def test_limits_follow_the_plan(hiplib, setter):
    out = (ctypes.c_uint32 * 4)()
    topk = (ctypes.c_uint32 * 4)()
    for kb, ib in WIDTHS:
        assert hiplib.rdst_hip_select_segments_limits(kb, ib, out) == OK and hiplib.rdst_hip_topk_segments_limits(kb, ib, topk) == OK
        assert tuple(out) == (topk[0], topk[1], topk[2], 32) == Q.limits(kb, bool(ib))
        for border in (1, topk[1], 1 << 22):
            assert setter(border) == OK
            assert hiplib.rdst_hip_select_segments_limits(kb, ib, out) == OK and tuple(out) == Q.limits(kb, bool(ib), border)
        assert setter(0) == OK
    for kb in (1, 2, 16):
        for ib in (4, 8):
            assert hiplib.rdst_hip_select_segments_limits(kb, ib, out) == UNSUPPORTED
    for kb in (0, 3, 32):
        assert hiplib.rdst_hip_select_segments_limits(kb, 0, out) == UNSUPPORTED
    assert hiplib.rdst_hip_select_segments_limits(4, 3, out) == ARG and hiplib.rdst_hip_select_segments_limits(4, 0, None) == ARG
    import rdst_amd
    assert rdst_amd.select_segments_limits("float64", 4) == (512, 8192, 1 << 17, 32) and rdst_amd.select_segments_limits("u128") == (256, 4096, 1 << 17, 32)


def test_scratch_bytes_is_pure_monotone_and_moves_with_the_setter(hiplib, setter):
    f = hiplib.rdst_hip_select_segments_scratch_bytes
    select = hiplib.rdst_hip_select_scratch_bytes
    for kb in (0, 3, 5, 32):
        assert f(10, 100, 5, kb, 0) == 0
    for kb in (1, 2, 16):
        assert f(10, 100, 5, kb, 4) == 0 and f(10, 100, 5, kb, 0) > 0
    assert f(0, 100, 5, 4, 0) == 0 and f(1 << 32, 100, 5, 4, 0) == 0 and f(10, 1 << 32, 5, 4, 0) == 0 and f(10, 100, 5, 4, 3) == 0
    for kb, ib in WIDTHS:
        _wm, bm, sm, _mr = Q.limits(kb, bool(ib))
        segs = (1, 2, 16, 17, 1000, 10**6, (1 << 32) - 1)
        longs = (0, 1, bm, bm + 1, sm, sm + 1, 1 << 24, (1 << 32) - 1)
        nrs = (1, 32, 33, 1 << 20)
        cube = [[[int(f(n, lg, nr, kb, ib)) for nr in nrs] for lg in longs] for n in segs]
        assert cube == [[[int(f(n, lg, nr, kb, ib)) for nr in nrs] for lg in longs] for n in segs]              # pure
        for i, n in enumerate(segs):
            table = (16 * n + 255) // 256 * 256
            for j, lg in enumerate(longs):
                for m, nr in enumerate(nrs):
                    assert cube[i][j][m] == table + (int(select(lg, nr, kb, ib, 0)) if lg > sm else 0), (kb, ib, n, lg, nr)
                    assert cube[i][j][m] % 256 == 0
                    if i: assert cube[i - 1][j][m] <= cube[i][j][m]                                            # monotone in all three
                    if j: assert cube[i][j - 1][m] <= cube[i][j][m]
                    if m: assert cube[i][j][m - 1] <= cube[i][j][m]
        lg = 4 * bm                                                         # the setter moves the border the function uses
        assert f(10, lg, 5, kb, ib) == 256
        assert setter(2 * bm) == OK
        assert f(10, lg, 5, kb, ib) == 256 + select(lg, 5, kb, ib, 0) and f(10, 2 * bm, 5, kb, ib) == 256
        assert setter(0) == OK
    import rdst_amd
    assert rdst_amd.select_segments_scratch_bytes(17, 100, 5, "uint32") == 512


def test_key_argument_errors_are_the_segmented_partial_sort_s(hiplib):
    """steps 1 and 2, whatever the other arguments are: the code and message rdst_hip_topk_segments_device gives"""
    buf, (k, o, i, s) = _pointers()
    before = buf.copy()
    _t, good = _table([0, 4, 8])
    calls = [
        (k, 8, 3, UNSIGNED, 3), (k, 8, 0, UNSIGNED, 0), (k, 8, 32, UNSIGNED, 32), (k, 8, 2, FLOAT, 2), (k, 8, 16, FLOAT, 16),
        (k, 8, 4, UNSIGNED, 0), (k, 8, 4, SIGNED, 3), (k, 8, 8, SIGNED, 4), (k, 8, 1, UNSIGNED, 2),
        (k, 8, 4, 4, 4), (k, 8, 4, -1, 4),
        (None, 8, 4, UNSIGNED, 4), (None, 1, 4, UNSIGNED, 4),
        (k + 2, 8, 4, UNSIGNED, 4), (k + 8, 8, 16, UNSIGNED, 16), (k + 1, 1, 2, SIGNED, 2),
        (k, 1 << 36, 4, UNSIGNED, 4),
    ]
    for keys, n, kb, kind, levels in calls:
        status = hiplib.rdst_hip_topk_segments_device(vp(keys), n, good, 2, 1, vp(o), None, 0, vp(s), BIG, kb, kind, levels, 0, None)
        assert status != OK
        msg = hiplib.rdst_hip_last_error()
        for off, nseg, specs, nr, out, idx, ib, scr, sb, flags in ((good, 2, GOOD, 3, o, i, 4, s, BIG, 0), (None, 3, [(3, 2, 0)], 1, None, None, 0, None, 0, 6),
                                                                   (good, 0, None, 0, o + 1, i + 1, 3, s + 1, 0, 0)):
            assert _seg(hiplib, keys, n, off, nseg, specs, nr, out, idx, ib, scr, sb, kb, kind, levels, flags) == status
            assert hiplib.rdst_hip_last_error() == msg
    for kb in (4, 16):                                                      # [u8; N] keys are not built
        assert _seg(hiplib, k, 8, None, 3, None, 2, None, None, 0, None, 0, kb, BYTES_BE, kb, 6) == UNSUPPORTED
    assert np.array_equal(buf, before)


def test_argument_errors_in_their_order(hiplib):
    buf, (k, o, i, s) = _pointers()
    before = buf.copy()
    n = 1000
    _t, good = _table([0, 10, 10, 700, 1000])
    _d, decreasing = _table([0, 10, 9, 700, 1000])
    _p, past = _table([0, 10, 10, 700, 1001])
    unset = object()

    def call(keys=k, n=n, off=good, nseg=4, specs=GOOD, nr=unset, out=o, idx=None, ib=0, scr=s, sb=BIG, kb=4, kind=UNSIGNED, flags=0):
        nr = (len(specs) if specs is not None else 0) if nr is unset else nr
        return _seg(hiplib, keys, n, off, nseg, specs, nr, out, idx, ib, scr, sb, kb, kind, kb, flags), hiplib.rdst_hip_last_error()

    # 2: len >= 2^32, before the flags, the table, the ranks and every pointer
    for bad_n in (1 << 32, (1 << 36) - 1):
        rc, msg = call(n=bad_n, flags=2, off=None, specs=None, nr=2, out=None, scr=None)
        assert rc == UNSUPPORTED and b"2^32" in msg
    # 3: unknown flag bits, before the no-ops
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        for nr, nseg in ((0, 4), (3, 0), (3, 4)):
            rc, msg = call(nr=nr, nseg=nseg, flags=flags, off=None, specs=None, out=None, scr=None)
            assert rc == ARG and b"flag" in msg
    # 4: no rank or no segment is a no-op: nothing else is looked at
    for flags in (0, LARGEST):
        assert call(nr=0, off=None, specs=None, out=None, idx=i + 1, ib=3, scr=None, sb=0, flags=flags)[0] == OK
        assert call(nseg=0, off=None, specs=[(3, 2, 0)], out=o + 1, idx=None, ib=99, scr=s + 1, sb=0, kb=16, flags=flags)[0] == OK
        assert call(nr=0, off=decreasing, out=None, scr=None, flags=flags)[0] == OK
    # 5: the table, before the ranks, the outputs and the scratch
    rc, msg = call(off=None, specs=None, nr=2, out=None, scr=None)
    assert rc == ARG and b"null offsets" in msg
    rc, msg = call(nseg=1 << 32, specs=None, nr=2, out=None, scr=None)
    assert rc == ARG and b"n_segments" in msg
    rc, msg = call(off=decreasing, specs=[(3, 2, 0)], out=None, idx=i + 1, ib=3, scr=None)
    assert rc == ARG and b"non-decreasing" in msg
    rc, msg = call(off=past, specs=None, nr=1, out=None, scr=None)
    assert rc == ARG and b"past len" in msg
    assert call(off=past, n=1001, scr=None)[0] == ARG and b"null scratch" in hiplib.rdst_hip_last_error()
    # 6: NULL ranks, then a bad spec; the message names the first
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
    # 7: the key output
    rc, msg = call(out=None, idx=i, ib=3, scr=None)
    assert rc == ARG and b"null key output" in msg
    for kb, off in ((2, 1), (4, 2), (8, 4), (16, 8)):
        rc, msg = call(out=o + off, kb=kb, idx=i, ib=3, scr=None)
        assert rc == ALIGN and b"key output" in msg
    # 8: the index output (only with an index: without one index_bytes is not looked at)
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
    # 9: the scratch; its need follows the table's longest segment (690 keys here)
    rc, msg = call(scr=None, sb=0)
    assert rc == ARG and b"null scratch" in msg
    for off in (1, 16, 128, 255):
        rc, msg = call(scr=s + off, sb=0)
        assert rc == ALIGN and b"scratch not aligned" in msg
    for kb, ib in ((4, 0), (4, 4), (8, 8), (16, 0), (1, 0)):
        need = int(hiplib.rdst_hip_select_segments_scratch_bytes(4, 690, 3, kb, ib))
        assert need == 256
        for sb in (0, 1, need - 1):
            rc, msg = call(idx=i if ib else None, ib=ib, kb=kb, sb=sb)
            assert rc == ARG and b"rdst_hip_select_segments_scratch_bytes" in msg, (kb, ib, sb)
    # a table of empty segments: everything is checked, nothing is done
    _e, empty = _table([5, 5, 5])
    assert call(off=empty, nseg=2, sb=255)[0] == ARG and call(off=empty, nseg=2, sb=256)[0] == OK
    assert np.array_equal(buf, before)


def test_a_far_segment_needs_its_part_of_the_scratch(hiplib, setter):
    buf, (k, o, _i, s) = _pointers()
    before = buf.copy()
    bm = S.block_max(4, False)
    n = 3 * bm
    _t, off = _table([0, 5, n])
    assert setter(bm) == OK
    need = int(hiplib.rdst_hip_select_segments_scratch_bytes(2, n - 5, 3, 4, 0))
    assert need == 256 + int(hiplib.rdst_hip_select_scratch_bytes(n - 5, 3, 4, 0, 0))
    assert _seg(hiplib, k, n, off, 2, GOOD, 3, o, None, 0, s, need - 1, 4, UNSIGNED, 4) == ARG
    assert b"rdst_hip_select_segments_scratch_bytes" in hiplib.rdst_hip_last_error()
    assert np.array_equal(buf, before)


def test_python_wrapper_refuses_device_operands_without_a_device():
    """the operand checks that need no device: what is not a HIP tensor is refused before the library is asked"""
    import torch
    import rdst_amd
    with pytest.raises(ValueError):
        rdst_amd.select_segments_device_tensor(torch.zeros(8, dtype=torch.int32), [0, 8], ranks=[0])
    with pytest.raises(ValueError):
        rdst_amd.select_rows_tensor(torch.zeros((2, 4), dtype=torch.int32), ranks=[0])


def test_cpp_source_compiles_and_links(tmp_path, hiplib):
    import subprocess
    src = os.path.join(ROOT, "tests", "cpp", "test_rdst_select_segments.cpp")
    exe = str(tmp_path / "test_rdst_select_segments")
    libdir = os.path.join(ROOT, "rdst_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-lrdst_hip",
                    f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    assert os.path.exists(exe)
