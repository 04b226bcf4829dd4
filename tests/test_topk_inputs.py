"""tests/topk_inputs.py is what it claims: the constants are the library's (each found on the line of rdst_topk.hip,
rdst_topk_layout.h or rdst_args.h that defines it, and in what rdst_hip_topk_limits answers), expected_topk agrees with the oracle's sorted output on the key bits
and is the stable argsort the contract names, the restated level loop agrees with a statement of the depth that has no
loop, and every case of tests/test_gpu_topk.py reaches the depth it is named for."""
import os
import re

import numpy as np
import pytest

import helpers as H
import topk_inputs as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "".join(open(os.path.join(ROOT, "rdst_amd", "csrc", name)).read() for name in ("rdst_topk.hip", "rdst_topk_layout.h", "rdst_args.h"))
UNSUPPORTED = -2


def _has(pattern):
    return re.search(pattern, SOURCE) is not None


def test_constants_are_the_library_s(hiplib):
    assert _has(rf"constexpr uint32_t COUNTERS = {T.COUNTERS};") and T.COUNTERS == 1 << T.DIGIT_BITS_WIDE
    assert _has(rf"constexpr uint32_t DIGIT_BITS_WIDE = {T.DIGIT_BITS_WIDE};") and _has(rf"constexpr uint32_t DIGIT_BITS_BYTE = {T.DIGIT_BITS_BYTE};")
    assert _has(rf"constexpr uint32_t POSITION_BITS = {T.POSITION_BITS};")
    assert _has(r"constexpr uint64_t DEFAULT_CAND_CAPACITY = 1ull << 20;") and T.DEFAULT_CAND_CAPACITY == 1 << 20
    assert _has(rf"constexpr int HIST_THREADS = {T.HIST_THREADS};") and _has(rf"constexpr int HIST_UNROLL = {T.HIST_UNROLL};")
    assert _has(rf"constexpr int BLOCKS_PER_CU = {T.BLOCKS_PER_CU};")
    import ctypes
    out = (ctypes.c_uint32 * 3)()
    for kb in (1, 2, 4, 8, 16):
        for ib in (0, 4, 8):
            rc = hiplib.rdst_hip_topk_limits(kb, ib, out)
            if ib and kb not in (4, 8):
                assert rc == UNSUPPORTED
                continue
            assert rc == 0 and tuple(out) == (T.digit_bits(kb), T.DEFAULT_CAND_CAPACITY, T.max_levels(kb, ib != 0)), (kb, ib)
    assert [T.max_levels(kb, False) for kb in (1, 2, 4, 8, 16)] == [1, 2, 3, 6, 11]
    assert T.max_levels(4, True) == 6 and T.max_levels(8, True) == 9


def test_level_shapes_cover_every_bit_once():
    for kb in (1, 2, 4, 8, 16):
        for indexed in (False, True):
            shapes = T.level_shapes(kb, indexed)
            assert len(shapes) == T.max_levels(kb, indexed)
            for field, bits in ((False, 8 * kb), (True, 32)):
                mine = [(s, b) for p, s, b in shapes if p == field]
                if field and not indexed:
                    assert mine == []
                    continue
                assert mine[0][0] + mine[0][1] == bits and mine[-1][0] == 0
                assert all(a[0] == b[0] + b[1] for a, b in zip(mine, mine[1:]))
                assert all(b <= T.digit_bits(kb) for _s, b in mine)


@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_expected_topk_is_the_front_of_the_oracle_s_sort(oracle, key, kb):
    n = 3001
    a = T.random_keys(n, key, 17 + kb)
    if not T.is_wide(key):
        a[::7] = a[3]                                     # equal keys
    s = a.copy()
    oracle.sort(s, kind=key if T.is_wide(key) else None)
    for k in (1, 2, 500, n - 1, n):
        ek, ei = T.expected_topk(a, k, False, key if T.is_wide(key) else None)
        assert np.array_equal(ek.view(np.uint8), s[:k].view(np.uint8)), k
        assert np.array_equal(a[ei].view(np.uint8), ek.view(np.uint8))
        lk, li = T.expected_topk(a, k, True, key if T.is_wide(key) else None)
        assert np.array_equal(lk.view(np.uint8), np.ascontiguousarray(s[::-1][:k]).view(np.uint8)), k
        assert np.array_equal(a[li].view(np.uint8), lk.view(np.uint8))


def test_expected_topk_is_stable_and_takes_the_lowest_positions():
    a = np.array([5, 1, 5, 0, 5, 1, 9, 5], dtype=np.int32)
    k, i = T.expected_topk(a, 5)
    assert list(k) == [0, 1, 1, 5, 5] and list(i) == [3, 1, 5, 0, 2]
    k, i = T.expected_topk(a, 4, largest=True)            # a stable argsort by the complement: NOT the reversed ascending argsort
    assert list(k) == [9, 5, 5, 5] and list(i) == [6, 0, 2, 4]
    f = np.array([0.0, -0.0, np.nan, -np.inf, 1.0], dtype=np.float32)
    k, i = T.expected_topk(f, 3)
    assert list(i) == [3, 1, 0]                           # -inf, -0.0, +0.0: distinct keys


def test_restated_loop_matches_the_direct_depth():
    rng = np.random.default_rng(5)
    for dtype in ("uint8", "uint16", "int32", "float32", "uint64", "float64"):
        kb = np.dtype(dtype).itemsize
        for j in range(kb + 1):
            a = T.shared_top(3000, dtype, j, 40 + j)
            for indexed in ((False, True) if kb in (4, 8) else (False,)):
                for cap in (1, 7, 64, 2999, 3000, 0):
                    for largest in (False, True):
                        k = int(rng.integers(1, 3001))
                        r = T.restate(a, k, largest, indexed, cap)
                        assert r["levels"] == T.direct_depth(a, k, largest, indexed, cap), (dtype, j, indexed, cap, k)
                        ek, ei = T.expected_topk(a, k, largest)
                        m = H.mapped_key(a)
                        m = ~m if largest else m
                        kth = m[ei[-1]]
                        if r["levels"] <= T.key_levels(kb):           # the prefix is a key prefix: everything below it is strictly before
                            assert r["c_below"] <= int((m < kth).sum())
                        assert r["c_below"] < k <= r["c_below"] + r["m"]
                        assert r["special"] == int(r["levels"] > T.key_levels(kb) or (not indexed and r["candidates"] == 0))


def test_depth_cases_reach_every_depth_they_are_named_for():
    seen = {}
    for dtype, j in T.depth_cases():
        kb = np.dtype(dtype).itemsize
        a = T.shared_top(T.DEPTH_LEN, dtype, j, 100 + j)
        m = H.mapped_key(a)
        assert len(np.unique(m >> np.array(8 * (kb - j), dtype=m.dtype))) == 1 if j else True
        k = T.DEPTH_LEN // 3
        base = T.restate(a, k, False, False, 64)
        # with 64 candidates the shared bytes cost their levels: at least the levels that lie wholly inside them, + 1
        assert base["levels"] >= min(8 * j // T.digit_bits(kb) + 1, T.key_levels(kb)), (dtype, j)
        assert base["levels"] == T.direct_depth(a, k, False, False, 64)
        seen.setdefault(dtype, set()).add(base["levels"])
        for cap in T.depth_capacities(base["m"]):
            r = T.restate(a, k, False, False, cap)
            assert r["levels"] == T.direct_depth(a, k, False, False, cap)
            if cap >= base["m"]:
                assert r["levels"] <= base["levels"]
            if cap == base["m"] - 1 and base["levels"] < T.key_levels(kb):
                assert r["levels"] > base["levels"] or base["m"] <= 64
        if j == kb:                                       # all keys equal: keys only ends in the fill, an index in position digits
            assert base["levels"] == T.key_levels(kb) and base["special"] == 1 and base["candidates"] == 0
            if kb in (4, 8):
                r = T.restate(a, k, False, True, 64)
                assert r["levels"] > T.key_levels(kb) and r["special"] == 1 and 1 <= r["candidates"] <= 64
    for dtype, depths in seen.items():
        kb = np.dtype(dtype).itemsize
        assert depths == set(range(1, T.key_levels(kb) + 1)), (dtype, depths)


def test_shared_top_wide_shares_what_it_says():
    for key in T.WIDE_KEYS:
        for bits in T.WIDE_DEPTH_BITS + (1, 63, 64, 65, 127):
            a = T.shared_top_wide(2000, key, bits, 9)
            v = T.mapped_ints(a, key)
            assert len({x >> (128 - bits) for x in v}) == 1
            if bits < 128:                                # the bit below the shared ones takes both values, the lowest one too
                assert len({(x >> (127 - bits)) & 1 for x in v}) == 2 and len({x & 1 for x in v}) == 2
            # mapped_ints, mapped_limbs and order_of say the same
            hi, lo = T.mapped_limbs(a, key)
            assert v == [(int(h) << 64) | int(l) for h, l in zip(hi.tolist(), lo.tolist())]
            assert list(T.order_of(a, key)) == sorted(range(2000), key=lambda i: v[i])
            w = T.mapped_ints(a, key, largest=True)
            assert w == [x ^ ((1 << 128) - 1) for x in v] and list(T.order_of(a, key, True)) == sorted(range(2000), key=lambda i: w[i])


@pytest.mark.parametrize("key", T.WIDE_KEYS)
def test_wide_depth_cases_reach_every_depth_and_the_fill(key):
    """the restated loop against the statement in Python integers (shared_counts_wide) on every case and capacity of
    test_every_depth_with_16_byte_keys — the level of bits [56, 68) takes its digit from both limbs — and the depths the
    cases are named for: 1 to 11 at capacity 64, none missing, and the fill"""
    assert T.key_levels(16) == 11 and T.level_shapes(16, False)[5] == (False, 56, 12) and T.level_shapes(16, False)[10] == (False, 0, 8)
    k = T.DEPTH_LEN // 3
    reached, fills, straddled = {}, set(), 0
    for kind, bits in T.wide_depth_cases():
        if kind != key:
            continue
        a = T.wide_depth_input(key, bits)
        for largest in (False, True):
            sizes = T.shared_counts_wide(a, k, largest, key)
            assert len(sizes) == 12 and sizes[0] == T.DEPTH_LEN and sizes == sorted(sizes, reverse=True) and sizes[-1] >= 1
            base = T.restate(a, k, largest, False, 64, key)
            for cap in T.depth_capacities(T.restate(a, k, False, False, 64, key)["m"]):
                r = T.restate(a, k, largest, False, cap, key)
                depth = T.direct_depth_wide(a, k, largest, cap, key, sizes)
                assert r["levels"] == depth, (key, bits, largest, cap, r, sizes)
                assert r["m"] == sizes[depth] and r["c_below"] < k <= r["c_below"] + r["m"]
                fill = depth == 11 and sizes[11] > cap
                assert (r["special"], r["candidates"]) == ((1, 0) if fill else (0, sizes[depth])), (key, bits, largest, cap)
                straddled += int(depth >= 6)
            reached.setdefault(largest, {})[bits] = base["levels"]
            if base["special"]:
                assert base["candidates"] == 0 and base["levels"] == 11
                fills.add((largest, bits))
    for largest in (False, True):
        for d in range(1, 12):
            assert reached[largest][12 * (d - 1)] == d, (key, largest, d, reached[largest])
        assert set(reached[largest].values()) == set(range(1, 12))
        assert reached[largest][60] == 6 and reached[largest][68] == 7 and reached[largest][128] == 11
        assert {(largest, 120), (largest, 128)} <= fills
    assert straddled > 0


@pytest.mark.parametrize("dtype,ib", T.FAR_CASES)
def test_far_cases_end_in_the_top_position_digit(dtype, ib):
    """all keys equal and a k-th element beyond position 2^20: every key level and every position level runs, the digit of
    the position bits 20 to 31 is 1, and one candidate is left"""
    a = T.far_input(dtype)
    kb = a.dtype.itemsize
    assert len(a) == T.FAR_LEN and len(np.unique(a)) == 1 and (T.FAR_K - 1) >> 20 == 1 and T.FAR_K < T.FAR_LEN < 1 << 21
    for cap in T.FAR_CAPACITIES:
        for largest in (False, True):
            assert np.array_equal(T.order_of(a, None, largest), np.arange(T.FAR_LEN))
            r = T.restate(a, T.FAR_K, largest, True, cap)
            assert r == {"levels": T.max_levels(kb, True), "c_below": T.FAR_K - 1, "candidates": 1, "special": 1, "m": 1}, (dtype, cap, r)
    assert [T.max_levels(np.dtype(d).itemsize, True) for d, _ in T.FAR_CASES] == [6, 9]


def test_tie_cases_tie_where_they_say():
    for dtype in ("uint32", "float32", "int64"):
        keys, k, at = T.tie_case(dtype, 3)
        m = H.mapped_key(keys)
        ek, ei = T.expected_topk(keys, k)
        kth = m[ei[-1]]
        tied = np.flatnonzero(m == kth)
        assert np.array_equal(tied, at) and len(at) == T.TIE_COUNT
        below = int((m < kth).sum())
        assert below < k < below + T.TIE_COUNT
        assert np.array_equal(ei[below:], at[:k - below])                   # the lowest positions win
        kb = np.dtype(dtype).itemsize
        for cap, fill in ((T.TIE_COUNT + 1, False), (T.TIE_COUNT, False), (T.TIE_COUNT - 1, True), (64, True)):
            r = T.restate(keys, k, False, False, cap)
            assert (r["candidates"] == 0 and r["special"] == 1) == fill, cap
            r = T.restate(keys, k, False, True, cap)
            assert (r["levels"] > T.key_levels(kb)) == fill and r["special"] == int(fill) and 1 <= r["candidates"] <= cap


def test_order_families_put_whole_waves_on_one_counter():
    for dtype in ("uint32", "float32", "uint64"):
        kb = np.dtype(dtype).itemsize
        n = 3 * T.block_batch(kb) + 17
        for name in T.ORDER_FAMILIES:
            m = H.mapped_key(T.order_sensitive(name, n, dtype))
            top = (m >> np.array(8 * kb - T.digit_bits(kb), dtype=m.dtype)).astype(np.int64)
            per_load = top[: n // (64 * T.vec(kb)) * 64 * T.vec(kb)].reshape(-1, 64, T.vec(kb))
            uniform = (per_load == per_load[:, :1, :]).all(axis=1).mean()
            assert uniform > 0.9, (dtype, name, uniform)
            if name == "ascending":
                assert (m[1:] > m[:-1]).all()
            if name == "descending":
                assert (m[1:] < m[:-1]).all()


def test_special_values_are_present():
    for dtype in ("float32", "float64"):
        a = T.float_specials(dtype, 5000, 1)
        u = H.uint_view(a)
        w = 8 * a.dtype.itemsize
        assert np.isnan(a).sum() >= 8 and len(np.unique(u[np.isnan(a)])) >= 8
        assert (np.signbit(a) & np.isnan(a)).any() and (~np.signbit(a) & np.isnan(a)).any()
        assert (u == 0).any() and (u == 1 << (w - 1)).any() and np.isposinf(a).any() and np.isneginf(a).any()
    for dtype in ("int8", "int32", "int64"):
        a = T.signed_extremes(dtype, 3000, 2)
        info = np.iinfo(dtype)
        assert (a == info.min).any() and (a == info.max).any() and (a == -1).any() and (a == 0).any()


def test_border_lengths_and_ks():
    for kb in (1, 2, 4, 8, 16):
        ls = T.border_lengths(kb)
        b = T.block_batch(kb)
        assert {1, 2, b - 1, b, b + 1} <= set(ls) and max(T.vec(kb) - 1, 1) in ls
        assert T.grid_worth(kb) == T.CUS * T.BLOCKS_PER_CU * T.HIST_THREADS * T.vec(kb) * T.HIST_UNROLL
    assert T.ks_for(1) == [1] and T.ks_for(2) == [1, 2] and T.ks_for(1000) == [1, 2, 63, 64, 65, 999, 1000] and T.ks_for(64) == [1, 2, 63, 64]
