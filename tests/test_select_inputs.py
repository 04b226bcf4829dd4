"""tests/select_inputs.py is what it claims: the constants are the library's (what rdst_hip_select_limits answers),
expected_select agrees with the oracle's sorted output on the key bits and is the stable argsort the contract names, the
restated round loop gives the same answers, every named case of tests/test_gpu_select.py reaches the depth, the group count,
the split or the exhaustion it is named for, and quantile_ranks indexes what numpy.quantile indexes."""
import ctypes
import os

import numpy as np
import pytest

import helpers as H
import select_inputs as S
import topk_inputs as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -2


def test_constants_are_the_library_s(hiplib):
    out = (ctypes.c_uint32 * 5)()
    for kb in (1, 2, 4, 8, 16):
        for ib in (0, 4, 8):
            rc = hiplib.rdst_hip_select_limits(kb, ib, out)
            if ib and kb not in (4, 8):
                assert rc == UNSUPPORTED
                continue
            assert rc == 0 and tuple(out) == (S.MAX_RANKS, S.digit0_bits(kb), S.DIGIT_BITS, S.DEFAULT_CAND_CAPACITY, S.max_levels(kb, ib != 0)), (kb, ib)
    assert [S.max_levels(kb, False) for kb in (1, 2, 4, 8, 16)] == [1, 2, 4, 8, 16]
    assert S.max_levels(4, True) == 8 and S.max_levels(8, True) == 12
    source = open(os.path.join(ROOT, "rdst_amd", "csrc", "rdst_select_layout.h")).read()
    assert f"constexpr uint32_t MAX_RANKS = {S.MAX_RANKS};" in source and "constexpr uint64_t DEFAULT_CAND_CAPACITY = 1ull << 24;" in source


def test_level_shapes_cover_every_bit_once():
    for kb in (1, 2, 4, 8, 16):
        for indexed in (False, True):
            shapes = S.level_shapes(kb, indexed)
            for field, bits in ((False, 8 * kb), (True, 32)):
                mine = [(s, b) for p, s, b in shapes if p == field]
                if field and not indexed:
                    assert mine == []
                    continue
                assert mine[0][0] + mine[0][1] == bits and mine[-1][0] == 0
                assert all(a[0] == b[0] + b[1] for a, b in zip(mine, mine[1:]))
            assert shapes[0][2] == S.digit0_bits(kb) and all(b <= S.DIGIT_BITS for _p, _s, b in shapes[1:])


@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_expected_select_indexes_the_oracle_s_sort(oracle, key, kb):
    n = 3001
    wide = key if T.is_wide(key) else None
    a = T.random_keys(n, key, 17 + kb)
    if not wide:
        a[::7] = a[3]                                     # equal keys
    s = a.copy()
    oracle.sort(s, kind=wide)
    ranks = [0, 1, 500, n - 1, 500, n // 2]
    ek, ei = S.expected_select(a, ranks, False, wide)
    assert np.array_equal(ek.view(np.uint8), s[ranks].view(np.uint8))
    assert np.array_equal(a[ei].view(np.uint8), ek.view(np.uint8))
    lk, li = S.expected_select(a, ranks, True, wide)
    assert np.array_equal(lk.view(np.uint8), s[[n - 1 - r for r in ranks]].view(np.uint8))
    assert np.array_equal(a[li].view(np.uint8), lk.view(np.uint8))
    if not wide:                                          # stable: among equal keys the positions ascend with the rank
        full_k, full_i = S.expected_select(a, list(range(n)), False, None)
        m = H.mapped_key(full_k)
        same = m[1:] == m[:-1]
        assert np.all(full_i[1:][same] > full_i[:-1][same]) and same.any()
        full_k, full_i = S.expected_select(a, list(range(n)), True, None)
        m = H.mapped_key(full_k)
        same = m[1:] == m[:-1]
        assert np.all(m[1:] <= m[:-1]) and np.all(full_i[1:][same] > full_i[:-1][same])


def _answers_agree(a, ranks, largest, indexed, cap, key=None):
    pos, states = S.restate(a, ranks, largest, indexed, cap, key)
    ek, ei = S.expected_select(a, ranks, largest, key)
    assert np.array_equal(np.ascontiguousarray(a[pos]).view(np.uint8), np.ascontiguousarray(ek).view(np.uint8))
    if indexed:
        assert np.array_equal(pos, ei)
    return states


@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_the_restated_loop_gives_the_expected_answers(key, kb):
    wide = key if T.is_wide(key) else None
    n = 6000
    a = T.random_keys(n, key, 5 + kb)
    a[n // 2:] = a[: n - n // 2]
    ranks = [int(r) for r in np.random.default_rng(kb).permutation(S.spaced_ranks(n, S.MAX_RANKS + 6) + [0, n - 1, 7, 7])]
    for largest in (False, True):
        for cap in (1, 64, 1000, 0):
            states = _answers_agree(a, ranks, largest, False, cap, wide)
            assert len(states) == 2
            if cap == 0:
                assert all(S.state_fields(st) == {"levels": 0, "groups": 1, "candidates": n, "exhausted": 0} for st in states)
            if key in [k for k, _ in T.INDEX_CASES]:
                for st in _answers_agree(a, ranks, largest, True, cap, None):
                    assert st["exhausted"] or st["candidates"] <= (cap or n)


def test_parting_cases_part_where_they_say():
    for dtype in ("uint32", "float64"):
        kl = S.key_levels(np.dtype(dtype).itemsize)
        for level in (1, 2, kl - 1):
            a, ranks = S.parting_input(dtype, level, 40 + level)
            st = _answers_agree(a, ranks, False, False, 1)[0]
            assert st["trace"][:level] == [1] * level and st["trace"][level] == 2 and st["exhausted"] == 1 and st["levels"] == kl
            st = _answers_agree(a, ranks, False, False, 64)[0]                            # (parting does not thin the groups: the levels go on)
            assert st["levels"] > level and st["groups"] == 2 and (st["exhausted"] or st["candidates"] <= 64)
            st = _answers_agree(a, ranks, False, True, 1)[0]
            assert st["levels"] > kl and st["exhausted"] in (0, 1) and st["groups"] == 2


def test_group_cases_have_the_groups_they_say():
    ranks = S.spaced_ranks(S.DEPTH_LEN, S.MAX_RANKS)
    for dtype in ("uint32", "int64"):
        st = _answers_agree(T.random_keys(S.DEPTH_LEN, dtype, 61), ranks, False, False, 3 * S.MAX_RANKS)[0]
        assert st["trace"][0] == S.MAX_RANKS and st["groups"] == S.MAX_RANKS
        st = _answers_agree(S.one_bucket_input(dtype, 62), ranks, False, False, 3 * S.MAX_RANKS)[0]
        assert st["trace"][0] == 1 and st["groups"] == S.MAX_RANKS and st["levels"] >= 2
    a, hr = S.heavy_input("uint32", 71)
    st = _answers_agree(a, hr, False, False, 64)[0]
    assert st["exhausted"] == 1 and st["candidates"] == 0 and st["groups"] == len(hr) - 2    # three ranks lie on the heavy value
    st = _answers_agree(a, hr, False, False, S.HEAVY_COUNT + 64)[0]
    assert st["exhausted"] == 0 and st["candidates"] >= S.HEAVY_COUNT
    st = _answers_agree(a, hr, False, True, 64)[0]
    assert st["levels"] > S.key_levels(4) and st["groups"] == len(hr)
    for count in (S.MAX_RANKS + 1, 2 * S.MAX_RANKS + 2):
        rk = S.spaced_ranks(S.DEPTH_LEN, count)
        assert [len(r) for r in S.rounds_of(rk)] == [S.MAX_RANKS] * (count // S.MAX_RANKS) + [count % S.MAX_RANKS]


def test_exhaustion_cases():
    n = 10_007
    for dtype in ("uint8", "uint32", "float64"):
        kb = np.dtype(dtype).itemsize
        a = np.full(n, H.random_bits(1, dtype, 3)[0], dtype=dtype)
        st = _answers_agree(a, [0, n // 2, n - 1], False, False, 64)[0]
        assert S.state_fields(st) == {"levels": S.key_levels(kb), "groups": 1, "candidates": 0, "exhausted": 1}
        if kb >= 4:
            st = _answers_agree(a, [0, n // 2, n - 1], False, True, 64)[0]
            assert st["levels"] > S.key_levels(kb) and st["groups"] == 3
    b = T.random_keys(S.DEPTH_LEN, "uint8", 91)
    st = _answers_agree(b, S.spaced_ranks(S.DEPTH_LEN, S.MAX_RANKS), False, False, 64)[0]
    assert st["levels"] == 1 and st["exhausted"] == 1
    for key in T.WIDE_KEYS:
        w = T.shared_top_wide(S.DEPTH_LEN, key, 128, 428)
        st = _answers_agree(w, [0, 5, S.DEPTH_LEN - 1], True, False, 1, key)[0]
        assert S.state_fields(st) == {"levels": 16, "groups": 1, "candidates": 0, "exhausted": 1}
        for bits in (60, 68):
            w = T.shared_top_wide(S.DEPTH_LEN, key, bits, 300 + bits)
            st = _answers_agree(w, [0, S.DEPTH_LEN // 3, S.DEPTH_LEN - 1], False, False, 64, key)[0]
            assert st["levels"] >= 1 + -(-(bits - 12) // 8) and st["exhausted"] == 0


def test_quantile_ranks_index_what_numpy_quantile_indexes():
    import rdst_amd
    rng = np.random.default_rng(1)
    qs = [0.0, 0.1, 0.25, 1 / 3, 0.5, 0.625, 0.9, 0.99, 1.0]
    for n in (1, 2, 3, 4, 5, 10, 11, 100, 101, 1000):
        a = rng.permutation(n).astype(np.float64) * 1.5
        s = np.sort(a)
        for method in ("lower", "higher", "nearest"):
            ranks = rdst_amd.quantile_ranks(n, qs, method)
            assert all(isinstance(r, int) for r in ranks)
            assert np.array_equal(s[ranks], np.quantile(a, qs, method=method)), (n, method)
    assert rdst_amd.quantile_ranks(10**9, 0.5) == [499_999_999] and rdst_amd.quantile_ranks(10**9, [0.5], "higher") == [500_000_000]
    with pytest.raises(ValueError):
        rdst_amd.quantile_ranks(10, [1.5])
    with pytest.raises(ValueError):
        rdst_amd.quantile_ranks(10, [0.5], "linear")
    with pytest.raises(ValueError):
        rdst_amd.quantile_ranks(0, [0.5])
