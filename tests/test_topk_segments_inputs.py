"""tests/topk_segments_inputs.py is what it claims: the expected result agrees with the oracle's sorted slice of every
segment (its first k_s; for largest its last k_s, reversed), the vectorised form agrees with the per-segment one, the plan
restated in numpy is rdst_topk_segments_plan's item for item, and the named cases of tests/test_gpu_topk_segments.py reach the
classes and depths they are named for.  The plan also runs as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/cpp/test_rdst_topk_segments_plan.cpp): host code only, never loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers as H
import topk_inputs as T
import topk_segments_inputs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = ((1, 0), (2, 0), (4, 0), (8, 0), (16, 0), (4, 4), (4, 8), (8, 4), (8, 8))
NAMES = {1: "uint8", 2: "uint16", 4: "uint32", 8: "uint64", 16: "u128"}


@pytest.fixture
def stream_max(hiplib):
    yield hiplib.rdst_hip_set_topk_segments_stream_max
    hiplib.rdst_hip_set_topk_segments_stream_max(0)


@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_expected_rows_are_the_ends_of_the_oracle_s_sorted_segments(oracle, key, kb):
    wide = key if T.is_wide(key) else None
    off, n = S.residue_table([0, 1, 2, 65, 700], kb)
    a = S.keys_for(n, key, 5 + kb)
    for k in (1, 2, 64, 699, 700, 701):
        for largest in (False, True):
            shape = (len(off) - 1, k, 2) if wide else (len(off) - 1, k)
            rows_k, rows_i = np.zeros(shape, dtype=a.dtype), np.full(shape[:2], -7, dtype=np.int64)
            S.expected_rows(a, off, k, largest, wide, rows_k, rows_i)
            per = S.expected(a, off, k, largest, wide)
            for s, (ek, ei) in enumerate(per):
                lo, hi = int(off[s]), int(off[s + 1])
                k_s = min(k, hi - lo)
                assert len(ei) == k_s and np.array_equal(rows_k[s, :k_s].view(np.uint8), ek.view(np.uint8)) and np.array_equal(rows_i[s, :k_s], ei)
                assert bool((rows_i[s, k_s:] == -7).all())
                srt = a[lo:hi].copy()
                if hi - lo > 1:
                    oracle.sort(srt, kind=wide)
                front = srt[::-1][:k_s] if largest else srt[:k_s]
                assert np.array_equal(ek.view(np.uint8), np.ascontiguousarray(front).view(np.uint8)), (s, k, largest)
                assert np.array_equal(a[lo:hi][ei].view(np.uint8), ek.view(np.uint8))           # the positions are local to the segment
                if not wide and k_s > 1:                                                          # equal keys in ascending position
                    same = H.mapped_key(ek)[1:] == H.mapped_key(ek)[:-1]
                    assert bool((np.diff(ei)[same] > 0).all())


@pytest.mark.parametrize("kb,ib", WIDTHS, ids=[f"k{kb}-i{ib}" for kb, ib in WIDTHS])
def test_numpy_plan_is_the_library_s(hiplib, stream_max, kb, ib):
    import rdst_amd
    rng = np.random.default_rng(kb * 10 + ib)
    wm, bm = S.wave_max(kb), S.block_max(kb, bool(ib))
    for border in (0, bm, 3 * bm, 1):
        assert stream_max(border) == 0
        assert rdst_amd.topk_segments_limits(NAMES[kb], ib) == S.limits(kb, bool(ib), border)
        tables = [np.cumsum([3] + S.segment_lengths(wm, bm) + [3 * bm, 3 * bm + 1, 1, 0, bm])]
        for _ in range(6):
            lens = np.concatenate([rng.integers(0, 4, 40), rng.integers(0, wm + 2, 40), rng.integers(wm, bm + 2, 20), rng.integers(bm, 5 * bm, 10)])
            tables.append(np.cumsum(np.concatenate([[rng.integers(0, 9)], rng.permutation(lens)])))
        for off in tables:
            for k in (0, 1, 77, bm, bm + 1, 1 << 40):
                got = rdst_amd.topk_segments_plan(off, int(off[-1]) + 2, k, NAMES[kb], ib)
                assert got == S.plan(off, k, kb, bool(ib), border), (border, k)
                items, counts, _far = got
                assert sorted(s for _st, _n, s in items) == [s for s in range(len(off) - 1) if off[s + 1] > off[s] and k]
                assert all(S.class_of(n, k, kb, bool(ib), border) == c for c in range(4) for _st, n, _s in items[sum(counts[:c]):sum(counts[:c + 1])])


def test_named_cases_reach_their_classes_and_depths():
    for key, kb in T.KEY_TYPES:
        for indexed in ((False, True) if kb in (4, 8) else (False,)):
            wm, bm = S.wave_max(kb), S.block_max(kb, indexed)
            lengths = S.segment_lengths(wm, bm)
            off, _n = S.residue_table(lengths, kb)
            starts = {}
            for lo, hi in zip(off[:-1], off[1:]):
                starts.setdefault(int(hi - lo), set()).add(int(lo) % (16 // kb))
            for n in lengths:
                if n >= 16 // kb or n == 0:
                    assert starts[n] >= set(range(16 // kb)), (key, n)               # every residue modulo the 16-byte vector
            ks = S.table_ks(wm, bm)
            assert {1, 2, 63, 64, 65, bm, bm + 1} <= set(ks)
            for k in (64, wm, 1024, bm):                                             # this k is n_s + 1, n_s and n_s - 1 of three rows
                assert {k - 1, k, k + 1} <= set(lengths) and k in ks                 # (and the row of 64 keys meets k = 63, 64, 65)
            seen = {k: {S.class_of(n, k, kb, indexed) for n in lengths if n} for k in ks}
            assert seen[1] == {0, 1, 2} and seen[bm] == {0, 1, 2} and seen[bm + 1] == {0, 1, 3}
            off, _n, sm = S.mixed_table(wm, bm, 3)
            for k in (1, 77, bm):
                assert all(c > 0 for c in S.plan(off, k, kb, indexed, sm)[1])
                assert int(off[0]) > 0 and 0 in (off[1:] - off[:-1])
    for dtype in ("uint16", "int32", "float32", "uint64", "float64"):
        kb = np.dtype(dtype).itemsize
        bm = S.block_max(kb, False)
        levels = T.key_levels(kb)
        depths = [S.stream_depth(S.shared_digits(2 * bm + 3, dtype, j, 40 + j), bm // 2 + 1, False, bm)[0] for j in range(levels + 1)]
        assert depths == [min(j + 1, levels) for j in range(levels + 1)], (dtype, depths)
        same = S.shared_digits(2 * bm + 3, dtype, levels, 40 + levels)
        assert len(np.unique(H.mapped_key(same))) == 1                               # digits exhausted with more than TILE ties
    for dtype, indexed in (("uint32", False), ("float32", True), ("int64", True), ("uint16", False)):
        bm = S.block_max(np.dtype(dtype).itemsize, indexed)
        for extra in (0, 1):
            a, k = S.stop_border(dtype, bm, 2 * bm + 3, extra, 5 + extra)
            levels, c_below, m = S.stream_depth(a, k, False, bm)
            assert levels == 1 + extra and (extra or c_below + m == bm)
    for dtype in ("uint32", "int32", "float64"):
        bm = S.block_max(np.dtype(dtype).itemsize, True)
        a, k, t_at = S.scattered_ties(dtype, 3 * bm + 5, bm, 21)
        levels, c_below, m = S.stream_depth(a, k, False, bm)
        assert levels == T.key_levels(a.dtype.itemsize) and c_below == bm // 4 and m == len(t_at) == 3 * bm // 2 and c_below + m > bm
        assert len(np.unique(a[t_at])) == 1 and c_below < k < c_below + m and bool((np.diff(t_at) > 1).any())


def test_plan_under_sanitizers(tmp_path):
    """rdst_segments.cpp with a main of its own, built with -fsanitize=address,undefined: a sanitizer report or a failed check
    is a non-zero exit"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "test_rdst_topk_segments_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_rdst_topk_segments_plan.cpp"), os.path.join(ROOT, "rdst_amd", "csrc", "rdst_segments.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
