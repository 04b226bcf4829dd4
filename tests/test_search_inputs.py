"""The inputs of the binary-search tests (tests/search_inputs.py) checked on the CPU: the constants against the source lines
they quote, the numpy statement of the result against a plain loop, the float keys, and that the haystacks and needles are
what their descriptions say."""
import os
import re

import numpy as np
import pytest

import search_inputs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = os.path.join(ROOT, "rdst_amd", "csrc", "rdst_search_layout.h")


def test_constants_are_the_source_s():
    lines = open(LAYOUT).read().splitlines()
    for name, value in (("THREADS", S.THREADS), ("SPLITTERS", S.SPLITTERS)):
        defining = [ln for ln in lines if re.match(rf"constexpr uint32_t {name} = ", ln)]
        assert len(defining) == 1 and defining[0].startswith(f"constexpr uint32_t {name} = {value};"), (name, defining)
    assert "constexpr uint32_t needles_per_thread(uint32_t elem_bytes) { return elem_bytes == 1 ? 16 : (elem_bytes == 16 ? 4 : 8); }" in lines
    assert S.NEEDLES_PER_THREAD == {b: (16 if b == 1 else 4 if b == 16 else 8) for b in (1, 2, 4, 8, 16)}
    assert "constexpr uint32_t needles_per_tile(uint32_t elem_bytes) { return THREADS * needles_per_thread(elem_bytes); }" in lines
    assert "constexpr uint32_t window(uint32_t elem_bytes) { return elem_bytes == 16 ? 2048 : (elem_bytes == 8 ? 4096 : 8192); }" in lines
    assert S.WINDOW == {b: (2048 if b == 16 else 4096 if b == 8 else 8192) for b in (1, 2, 4, 8, 16)}
    kernel = open(os.path.join(ROOT, "rdst_amd", "csrc", "rdst_search.hip")).read()
    assert f"constexpr uint32_t ERR_LEN_PAST_CAPACITY = {S.ERR_LEN_PAST_CAPACITY};" in kernel
    assert [S.tile(b) for b in (1, 2, 4, 8, 16)] == [4096, 2048, 2048, 2048, 1024]


def test_limits_are_the_constants(hiplib):
    import rdst_amd
    for key, kb in S.KEY_CASES:
        assert rdst_amd.search_limits(key) == (S.tile(kb), S.SPLITTERS, S.WINDOW[kb])


@pytest.mark.parametrize("key,kb", S.KEY_CASES)
def test_numpy_statement_against_a_loop(key, kb):
    for m in (0, 1, 2, 7, 40):
        for distinct in (1, 3, None):
            hay = S.haystack(key, m, seed=kb, distinct=distinct)
            assert len(hay) == m and (hay.shape == (m, 2) if S.wide(key) else hay.dtype == np.dtype(key))
            hm = [int(x) for x in S.mapped(hay, key)]
            assert hm == sorted(hm) and all(x % 2 == 0 for x in hm)
            for n in (1, 5, 30):
                needles = S.needles_for(hay, key, n, seed=n)
                assert len(needles) == n
                lower, upper = S.expected(hay, needles, key)
                loop_lower, loop_upper = S.expected_by_loop(hay, needles, key)
                assert lower.tolist() == loop_lower and upper.tolist() == loop_upper
                for cut in (0, m // 2):
                    lo, up = S.expected(hay, needles, key, cut)
                    assert (lo.tolist(), up.tolist()) == tuple(S.expected_by_loop(hay, needles, key, cut))


@pytest.mark.parametrize("key,kb", S.KEY_CASES)
def test_needles_are_what_their_description_says(key, kb):
    """present keys, keys between two neighbours, keys below the first and above the last, the extremes: all of them occur"""
    hay = S.haystack(key, 500, seed=1)
    needles = S.needles_for(hay, key, 300, seed=2)
    lower, upper = S.expected(hay, needles, key)
    q = [int(x) for x in S.mapped(needles, key)]
    hm = [int(x) for x in S.mapped(hay, key)]
    assert np.any(upper > lower) and np.any((upper == lower) & (lower > 0) & (lower < 500))      # present, and absent in between
    assert np.any(upper == 0) and np.any(lower == 500)                                             # below the first, above the last
    assert 0 in q and (1 << (8 * kb)) - 1 in q and hm[0] in q and hm[-1] in q
    assert np.any(upper - lower > 1) or kb >= 4                                                    # repeated keys (narrow keys: surely)
    back = S.mapped(S.from_mapped(q, key), key)
    assert [int(x) for x in back] == q                                                             # from_mapped inverts mapped


def test_float_cases_go_by_bits():
    cases = S.float_cases()
    assert sorted(cases) == ["float32", "float64"]
    for name, (hay, needles, lower, upper) in cases.items():
        got_lower, got_upper = S.expected(hay, needles, name)
        assert got_lower.tolist() == lower and got_upper.tolist() == upper, name
        assert (lower, upper) == tuple(S.expected_by_loop(hay, needles, name))
        assert np.isnan(hay[[0, 1, 9, 10]]).all() and hay[4] == hay[5] == 0 and np.signbit(hay[4]) and not np.signbit(hay[5])
        # what ordering by value cannot do: -0.0 and +0.0 are one place apart, every NaN has a place of its own
        assert lower[4] + 1 == lower[5] and len({lower[0], lower[1], lower[9], lower[10]}) == 4


def test_lengths_and_counts_sit_on_the_borders():
    for kb in (1, 2, 4, 8, 16):
        s, w, t = S.SPLITTERS, S.WINDOW[kb], S.tile(kb)
        assert S.haystack_lengths(kb) == (0, 1, 2, s - 1, s, s + 1, w - 1, w, w + 1, 3 * w + 5)
        assert S.needle_counts(kb) == (1, t - 1, t, t + 1, 3 * t + 5)
