"""The work list of the segmented sort (rdst_segments_plan, rdst_hip_sort_segments_limits; host only): one item per segment
of at least two keys, in the class its length and the limits dictate, in the documented order — wave class in segment
order, block class longest first with ties in segment order, long class in segment order — and the longest long segment
as the scratch the entry needs.  The same tables go through a stand-alone build of rdst_segments.cpp under the address
and undefined-behaviour sanitizers (tests/cpp/test_rdst_segments.cpp): host code only, never loaded into Python."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RDST_OK, RDST_ERR_ARG, RDST_ERR_UNSUPPORTED = 0, -1, -2
KEYS_ONLY_FLOOR = {1: 16384, 2: 16384, 4: 16384, 8: 8192, 16: 4096}   # today's one-workgroup limit
WIDTHS = [(kb, 0) for kb in (1, 2, 4, 8, 16)] + [(4, 4), (4, 8), (8, 4), (8, 8)]


def _item_type():
    from rdst_amd._lib import SegmentItemC   # rdst_segment_item: { u64 start; u32 len; u32 seg; }
    assert ctypes.sizeof(SegmentItemC) == 16
    return SegmentItemC


def limits(lib, kb, vb):
    out = (ctypes.c_uint32 * 2)()
    assert lib.rdst_hip_sort_segments_limits(kb, vb, out) == RDST_OK
    return int(out[0]), int(out[1])


def plan(lib, offsets, n, kb, vb, capacity=None):
    """(rc, items, counts, tmp_elems); offsets: a list, or None for a NULL pointer (then `capacity` segments are claimed)"""
    if offsets is None:
        offp, nseg = None, capacity
    else:
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        offp, nseg = off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(off) - 1
    cap = nseg if capacity is None else capacity
    items = (_item_type() * max(1, cap))()
    counts = (ctypes.c_uint64 * 3)(7, 7, 7)
    tmp = ctypes.c_uint64(7)
    rc = lib.rdst_segments_plan(offp, nseg, n, kb, vb, items, cap, counts, ctypes.byref(tmp))
    total = sum(counts)
    return rc, [(it.start, it.len, it.seg) for it in items[:min(total, cap)]], [int(c) for c in counts], int(tmp.value)


def expected(offsets, wave_max, block_max):
    """the documented list, from the lengths alone"""
    segs = [(int(offsets[s]), int(offsets[s + 1] - offsets[s]), s) for s in range(len(offsets) - 1)]
    segs = [x for x in segs if x[1] >= 2]
    wave = [x for x in segs if x[1] <= wave_max]
    block = sorted((x for x in segs if wave_max < x[1] <= block_max), key=lambda x: (-x[1], x[2]))
    long_ = [x for x in segs if x[1] > block_max]
    return wave + block + long_, [len(wave), len(block), len(long_)], max((x[1] for x in long_), default=0)


def hand_made(wave_max, block_max):
    lengths = [0, 0, 1, 2, 3, 63, 64, 65, wave_max - 1, wave_max, wave_max + 1, 1023, 1024, 1025, block_max - 1, block_max,
               block_max + 1, 2 * block_max + 17, block_max, wave_max + 1, 0]
    return np.concatenate([[5], 5 + np.cumsum(lengths)]).astype(np.uint64)


def random_table(rng, wave_max, block_max):
    nseg = int(rng.integers(1, 400))
    kind = rng.integers(0, 4, size=nseg)
    lengths = np.where(kind == 0, rng.integers(0, 4, size=nseg),
                       np.where(kind == 1, rng.integers(0, wave_max + 2, size=nseg),
                                np.where(kind == 2, rng.integers(wave_max, block_max + 2, size=nseg),
                                         rng.integers(block_max, 3 * block_max, size=nseg))))
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64) + np.uint64(rng.integers(0, 9))   # (a head gap of 0..8)


@pytest.mark.parametrize("kb,vb", WIDTHS)
def test_limits(hiplib, kb, vb):
    wave_max, block_max = limits(hiplib, kb, vb)
    assert wave_max >= 64 and wave_max < block_max
    assert block_max >= (KEYS_ONLY_FLOOR[kb] if vb == 0 else 4096)


@pytest.mark.parametrize("kb,vb", [(3, 0), (0, 0), (32, 0), (2, 4), (16, 8), (4, 2), (8, 16), (4, 3)])
def test_limits_unsupported_widths(hiplib, kb, vb):
    out = (ctypes.c_uint32 * 2)()
    assert hiplib.rdst_hip_sort_segments_limits(kb, vb, out) == RDST_ERR_UNSUPPORTED
    assert hiplib.rdst_hip_last_error()
    counts = (ctypes.c_uint64 * 3)()
    tmp = ctypes.c_uint64(0)
    off = (ctypes.c_uint64 * 2)(0, 10)
    assert hiplib.rdst_segments_plan(off, 1, 10, kb, vb, None, 0, counts, ctypes.byref(tmp)) == RDST_ERR_UNSUPPORTED


@pytest.mark.parametrize("kb,vb", WIDTHS)
def test_hand_made_table(hiplib, kb, vb):
    wave_max, block_max = limits(hiplib, kb, vb)
    off = hand_made(wave_max, block_max)
    rc, items, counts, tmp = plan(hiplib, off, int(off[-1]) + 7, kb, vb)
    exp_items, exp_counts, exp_tmp = expected(off, wave_max, block_max)
    assert rc == RDST_OK
    assert counts == exp_counts and counts[2] == 2 and tmp == exp_tmp == 2 * block_max + 17
    assert items == exp_items
    # the block class: longest first, ties in segment order
    block = items[counts[0]:counts[0] + counts[1]]
    assert [b[1] for b in block] == sorted((b[1] for b in block), reverse=True)
    assert all(a[2] < b[2] for a, b in zip(block, block[1:]) if a[1] == b[1])


@pytest.mark.parametrize("kb,vb", [(4, 0), (8, 0), (16, 0), (1, 0), (4, 4), (8, 8)])
def test_random_tables(hiplib, kb, vb):
    wave_max, block_max = limits(hiplib, kb, vb)
    rng = np.random.default_rng(1000 * kb + vb)
    for _ in range(25):
        off = random_table(rng, wave_max, block_max)
        rc, items, counts, tmp = plan(hiplib, off, int(off[-1]) + int(rng.integers(0, 3)), kb, vb)
        exp_items, exp_counts, exp_tmp = expected(off, wave_max, block_max)
        assert rc == RDST_OK
        assert counts == exp_counts and tmp == exp_tmp
        assert items == exp_items
        assert sorted(x[2] for x in items) == [s for s in range(len(off) - 1) if off[s + 1] - off[s] >= 2]


def test_zero_segments_and_all_empty(hiplib):
    rc, items, counts, tmp = plan(hiplib, None, 100, 4, 0, capacity=0)      # n_segments == 0: NULL offsets are fine
    assert (rc, items, counts, tmp) == (RDST_OK, [], [0, 0, 0], 0)
    rc, items, counts, tmp = plan(hiplib, [3], 100, 4, 0)
    assert (rc, items, counts, tmp) == (RDST_OK, [], [0, 0, 0], 0)
    rc, items, counts, tmp = plan(hiplib, [0, 0, 1, 1, 2, 2, 2], 2, 8, 4)    # lengths 0 and 1 only
    assert (rc, items, counts, tmp) == (RDST_OK, [], [0, 0, 0], 0)
    counts = (ctypes.c_uint64 * 3)(7, 7, 7)
    t = ctypes.c_uint64(7)
    off = (ctypes.c_uint64 * 3)(0, 1, 1)
    assert hiplib.rdst_segments_plan(off, 2, 1, 4, 0, None, 0, counts, ctypes.byref(t)) == RDST_OK   # nothing to list: no table needed


def test_capacity_too_small_still_reports_the_counts(hiplib):
    wave_max, block_max = limits(hiplib, 4, 0)
    off = hand_made(wave_max, block_max)
    _items, exp_counts, exp_tmp = expected(off, wave_max, block_max)
    rc, _, counts, tmp = plan(hiplib, off, int(off[-1]), 4, 0, capacity=sum(exp_counts) - 1)
    assert rc == RDST_ERR_ARG and hiplib.rdst_hip_last_error()
    assert counts == exp_counts and tmp == exp_tmp
    rc, _, counts, tmp = plan(hiplib, off, int(off[-1]), 4, 0, capacity=0)
    assert rc == RDST_ERR_ARG and counts == exp_counts and tmp == exp_tmp
    assert plan(hiplib, off, int(off[-1]), 4, 0, capacity=sum(exp_counts))[0] == RDST_OK


def test_bad_offsets(hiplib):
    rc, _, counts, _tmp = plan(hiplib, [0, 10, 9, 20], 20, 4, 0)
    assert rc == RDST_ERR_ARG and b"non-decreasing" in hiplib.rdst_hip_last_error() and counts == [0, 0, 0]
    rc, _, _, _ = plan(hiplib, [0, 10, 21], 20, 4, 0)
    assert rc == RDST_ERR_ARG and b"past len" in hiplib.rdst_hip_last_error()
    rc, _, _, _ = plan(hiplib, None, 20, 4, 0, capacity=3)
    assert rc == RDST_ERR_ARG and b"null offsets" in hiplib.rdst_hip_last_error()
    assert plan(hiplib, [0, 10, 20], 20, 4, 0)[0] == RDST_OK


def test_plan_under_sanitizers(tmp_path):
    """rdst_segments.cpp with a main of its own, built with -fsanitize=address,undefined: the same tables, checked in C++
    against the documented order; a sanitizer report or a failed check is a non-zero exit"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "test_rdst_segments")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_rdst_segments.cpp"), os.path.join(ROOT, "rdst_amd", "csrc", "rdst_segments.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
