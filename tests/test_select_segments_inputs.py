"""CPU-side checks of the segmented select's rank rule and of the case tables its GPU tests use
(tests/select_segments_inputs.py): rdst_rank_for_length against the rule restated in exact rationals and against
quantile_ranks where the float product is exact, half-way cases to even, the tables for what they claim, and the rule's edges
in a stand-alone build of rdst_segments.cpp under the address and undefined-behaviour sanitizers
(tests/cpp/test_rdst_select_ranks.cpp): host code only, never loaded into Python."""
import ctypes
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import helpers as H
import select_segments_inputs as Q
import topk_inputs as T
import topk_segments_inputs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
TOP = (1 << 32) - 1
LENGTHS = (1, 2, 3, 4, 5, 1000, TOP)


def _c_rank(lib, spec, n):
    from rdst_amd import _lib
    out = ctypes.c_uint64((1 << 64) - 1)
    rc = lib.rdst_rank_for_length(ctypes.byref(_lib.RankSpecC(spec[0], spec[1], spec[2], 0)), n, ctypes.byref(out))
    assert rc in (0, 1), (spec, n, rc)
    assert rc == 1 or out.value == (1 << 64) - 1                            # no rank: nothing is written
    return out.value if rc == 1 else None


def test_rank_rule_against_the_restatement(hiplib):
    quantiles = ((0, 1), (1, 1), (1, 2), (1, 3), (9, 10), (TOP, TOP), (2, 3), (1, TOP), (TOP - 1, TOP), (0, TOP), (7, 7))
    for n in LENGTHS:
        for num, den in quantiles:
            for mode in (Q.LOWER, Q.HIGHER, Q.NEAREST):
                want = Q.rank_of((num, den, mode), n)
                assert want is not None and 0 <= want < n
                assert _c_rank(hiplib, (num, den, mode), n) == want, (num, den, mode, n)
        for r in (0, n - 1, n, n + 1, TOP):
            if r <= TOP:
                want = r if r < n else None
                assert Q.rank_of((r, 0, 0), n) == want and _c_rank(hiplib, (r, 0, 0), n) == want, (r, n)
    for spec in ((0, 0, 0), (1, 2, 0), (1, 1, 2)):
        assert Q.rank_of(spec, 0) is None and _c_rank(hiplib, spec, 0) is None           # an empty segment has no element
    # the rule itself, where it can be read off: the ends, the three roundings of 4.5 and of 4.4
    assert [Q.rank_of((1, 2, m), 10) for m in (0, 1, 2)] == [4, 5, 4] and [Q.rank_of((1, 2, m), 12) for m in (0, 1, 2)] == [5, 6, 6]
    assert [Q.rank_of((4, 10, m), 12) for m in (0, 1, 2)] == [4, 5, 4] and [Q.rank_of((6, 10, m), 12) for m in (0, 1, 2)] == [6, 7, 7]


def test_bad_specs_are_argument_errors(hiplib):
    from rdst_amd import _lib
    out = ctypes.c_uint64(0)
    for num, den, mode, reserved in ((3, 2, 0, 0), (TOP, TOP - 1, 0, 0), (1, 2, 3, 0), (1, 2, TOP, 0), (1, 2, 0, 1), (0, 0, 0, TOP), (5, 0, 1, 0), (5, 0, 2, 0)):
        assert not Q.spec_ok((num, den, mode)) or reserved
        assert hiplib.rdst_rank_for_length(ctypes.byref(_lib.RankSpecC(num, den, mode, reserved)), 10, ctypes.byref(out)) == ARG
        assert b"rank spec" in hiplib.rdst_hip_last_error()
    good = _lib.RankSpecC(1, 2, 0, 0)
    assert hiplib.rdst_rank_for_length(None, 10, ctypes.byref(out)) == ARG and hiplib.rdst_rank_for_length(ctypes.byref(good), 10, None) == ARG
    assert hiplib.rdst_rank_for_length(ctypes.byref(good), (1 << 32) + 1, ctypes.byref(out)) == ARG
    assert hiplib.rdst_rank_for_length(ctypes.byref(good), 1 << 32, ctypes.byref(out)) == 1 and out.value == (1 << 31) - 1


def test_rank_rule_against_quantile_ranks_where_floats_are_exact(hiplib):
    """a denominator that is a power of two, and (n - 1) * num below 2^53: numpy's float virtual index is exact"""
    import rdst_amd
    for n in (1, 2, 3, 4, 5, 7, 1000, 1001, 65536, 10**6 + 3):
        for den in (1, 2, 4, 8, 1024):
            nums = sorted({0, 1, den // 2, den - 1, den} & set(range(den + 1)))
            for method, mode in Q.MODES.items():
                want = rdst_amd.quantile_ranks(n, [num / den for num in nums], method)
                assert [Q.rank_of((num, den, mode), n) for num in nums] == want, (n, den, method)
                assert [_c_rank(hiplib, (num, den, mode), n) for num in nums] == want
                assert [rdst_amd.rank_for_length(n, quantile=(num, den), method=method) for num in nums] == want


def test_half_way_cases_go_to_even(hiplib):
    for n in range(1, 40):
        got = _c_rank(hiplib, (1, 2, Q.NEAREST), n)
        if n % 2 == 0:                                                      # the virtual index (n - 1) / 2 ends in .5
            assert got % 2 == 0 and abs(Fraction(n - 1, 2) - got) == Fraction(1, 2)
        assert got == Q.rank_of((1, 2, Q.NEAREST), n) == int(np.around((n - 1) / 2))
    assert [_c_rank(hiplib, (k, 8, Q.NEAREST), 5) for k in range(9)] == [0, 0, 1, 2, 2, 2, 3, 4, 4]  # virtual k / 2


def test_python_operands():
    import rdst_amd
    from rdst_amd import radix_sort as R
    assert R._rank_specs([3, 0], [0.1, Fraction(2, 3), (5, 10), 1, 0.0], "nearest") == [(3, 0, 0), (0, 0, 0), (1, 10, 2), (2, 3, 2), (5, 10, 2), (1, 1, 2), (0, 1, 2)]
    assert R._rank_specs(np.array([7]), np.array([0.25]), "higher") == [(7, 0, 0), (1, 4, 1)]
    for bad in ([1.5], [-0.1], [(3, 2)], [(1, 0)], [Fraction(5, 4)], [(1, 1 << 32)], [1 / 3]):   # 1 / 3: its shortest decimal has 16 digits
        with pytest.raises(ValueError):
            R._rank_specs(None, bad, "lower")
    for bad in ([-1], [1 << 32]):
        with pytest.raises(ValueError):
            R._rank_specs(bad, None, "lower")
    with pytest.raises(ValueError):
        R._rank_specs([1], None, "linear")
    assert rdst_amd.rank_for_length(10, rank=9) == 9 and rdst_amd.rank_for_length(10, rank=10) is None and rdst_amd.rank_for_length(0, quantile=0.5) is None
    assert rdst_amd.rank_for_length(11, quantile=0.1) == 1 and rdst_amd.rank_for_length(12, quantile=0.1, method="higher") == 2
    with pytest.raises(ValueError):
        rdst_amd.rank_for_length(10)


def test_case_tables_are_what_they_claim(hiplib):
    out = (ctypes.c_uint32 * 4)()
    for kb, indexed in ((1, False), (2, False), (4, False), (8, False), (16, False), (4, True), (8, True)):
        wm, bm, sm, mr = Q.limits(kb, indexed)
        assert hiplib.rdst_hip_select_segments_limits(kb, 4 if indexed else 0, out) == 0 and tuple(out) == (wm, bm, sm, mr)   # the tables' tile is the library's
        assert mr == 32 and sm == 1 << 17 and bm == S.block_max(kb, indexed)
        lengths = S.segment_lengths(wm, bm)
        assert {0, 1, wm - 1, wm, wm + 1, bm - 1, bm, bm + 1} <= set(lengths)
        off, n = S.residue_table(lengths, kb)
        assert int(off[0]) > 0 and n > int(off[-1])                         # a gap before the first border and behind the last
        assert 0 in (off[1:] - off[:-1])
        sets = Q.rank_sets(wm)
        assert len(sets[3]) == 5 and len(set(sets[3])) == 4 and all(Q.spec_ok(s) for ss in sets for s in ss)
        lens = {int(x) for x in off[1:] - off[:-1]}
        assert any(Q.rank_of((wm, 0, 0), x) is None for x in lens if x) and any(Q.rank_of((wm, 0, 0), x) == wm for x in lens)
    for count in (33, 65):
        specs = Q.many_specs(count, count)
        assert len(specs) == count and all(Q.spec_ok(s) for s in specs) and sum(1 for s in specs if s[1] == 0) == 3
        assert {s[2] for s in specs} == {0, 1, 2}
    # (a) every select depth
    for dtype in ("uint16", "int32", "float32", "uint64", "float64"):
        kb = np.dtype(dtype).itemsize
        bm = S.block_max(kb, False)
        levels = T.key_levels(kb)
        n = 2 * bm + 3
        depths = [Q.stream_select(S.shared_digits(n, dtype, j, 40 + j), n // 2, False, bm)[0] for j in range(levels + 1)]
        assert depths == [min(j + 1, levels) for j in range(levels + 1)], (dtype, depths)
        _lv, c_below, m = Q.stream_select(S.shared_digits(n, dtype, levels, 40 + levels), n // 2, False, bm)
        assert (c_below, m) == (0, n)                                       # digits exhausted with more than TILE equal keys
    # (b) exactly TILE keys on the final prefix, and TILE + 1; more keys before the prefix than the partial sort would stage
    for dtype, indexed in (("uint32", False), ("float32", True), ("int64", True), ("uint16", False)):
        bm = S.block_max(np.dtype(dtype).itemsize, indexed)
        for extra in (0, 1):
            a, r = Q.prefix_border(dtype, bm, 2 * bm + 3, extra, 5 + extra)
            levels, c_below, m = Q.stream_select(a, r, False, bm)
            assert levels == 1 + extra and (extra or m == bm) and c_below <= r < c_below + m
            one = Q.stream_select(a, r, False, 1 << 30)
            assert one == (0, 0, len(a))
            assert Q.stream_select(a, r, False, bm + extra)[0] == 1 and Q.stream_select(a, r, False, bm + extra)[2] == bm + extra
            assert c_below + m > bm or extra
    # (c) ranks that share one stage, and ranks 0 and n - 1 with disjoint prefixes
    bm = S.block_max(4, False)
    a = T.random_keys(2 * bm + 3, "uint32", 77)
    n = len(a)
    _lv, c_below, m = Q.stream_select(a, n // 2, False, bm)
    assert m >= 3 and Q.descents(a, [c_below, c_below + 1, c_below + m - 1], False, bm) == 1
    assert Q.descents(a, [0, n - 1], False, bm) == 2 and Q.stream_select(a, 0, False, bm)[1] == 0
    assert Q.stream_select(a, n - 1, False, bm)[1] + Q.stream_select(a, n - 1, False, bm)[2] == n
    # (d) windows of an all-equal segment
    for kb in (4, 8):
        tile = S.block_max(kb, True)
        ranks = Q.window_ranks(tile)
        assert sorted({r // tile for r in ranks}) == [0, 1, 2, 3] and max(ranks) < 3 * tile + 5
        equal = np.full(3 * tile + 5, 7, dtype=f"u{kb}")
        assert Q.descents(equal, ranks, False, tile) == 4
    # (e) the ranks land on the zeros and the NaNs
    for dtype in ("float32", "float64"):
        bm = S.block_max(np.dtype(dtype).itemsize, False)
        a, ranks = Q.float_zero_nan_segment(dtype, 2 * bm + 3, 9)
        got = a[T.order_of(a)][ranks]
        u = got.view(f"u{a.dtype.itemsize}")
        assert len(ranks) == 12 and len(set(ranks)) == 12
        assert bool((got[:4] == 0).all()) and bool(np.signbit(got[:2]).all()) and not bool(np.signbit(got[2:4]).any())
        assert bool(np.isnan(got[4:]).all()) and len(set(u[4:].tolist())) == 4


def test_rank_rule_under_sanitizers(tmp_path):
    """rdst_segments.cpp with a main of its own, built with -fsanitize=address,undefined: a sanitizer report or a failed check
    is a non-zero exit"""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "test_rdst_select_ranks")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_rdst_select_ranks.cpp"), os.path.join(ROOT, "rdst_amd", "csrc", "rdst_segments.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
