"""The inputs of tests/test_gpu_keys.py, checked where no device is needed: the tiles are the library's (every constant quoted
in tests/devlen_inputs.py found on the line of rdst_kernels.hip that defines it), each skipped-level case holds exactly the
constant levels it names and both parities of the passes left occur per type, the copy-back inputs leave an odd number of
passes at every remainder of n * sizeof(K) modulo 16, the heavy-digit inputs hold single-digit rounds and runs longer than a
wave's span at the keys-only tile sizes, and the limb forms of the builders agree with Python's big integers."""
import os
import re

import numpy as np
import pytest

import devlen_inputs as D
import helpers as H
import keys_inputs as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = open(os.path.join(ROOT, "rdst_amd", "csrc", "rdst_kernels.hip")).read()


def _has(pattern):
    return re.search(pattern, SOURCE) is not None


def test_tiles_are_the_library_s():
    # the default pass shapes: 12 waves; keys per 8-byte thread 12 / 14 / 11 / 10 for the shapes 2 to 5
    for row in (r"\{12, 24, 12, 2\},  // 2:", r"\{12, 28, 14, 2\},  // 3:", r"\{12, 22, 11, 1\},  // 4:", r"\{12, 20, 10, 1\},  // 5:"):
        assert _has(row), row
    assert D.PASS_THREADS == 12 * 64
    assert _has(r"if \(elem_bytes == 8\) return mapped \? 5 : 3;") and _has(r"if \(elem_bytes <= 4 && n \* elem_bytes < \(1ull << 32\)\) return 4;")
    assert _has(r"elem_bytes <= 4 \? kpt8 \* 2 : \(elem_bytes == 8 \? kpt8 : \(kpt8 / 2\) & ~1\)")
    assert D.PASS_KPT == {(1, False): 11 * 2, (2, False): 11 * 2, (4, False): 11 * 2, (1, True): 11 * 2, (2, True): 11 * 2, (4, True): 11 * 2,
                          (8, False): 14, (8, True): 10, (16, False): (12 // 2) & ~1, (16, True): (12 // 2) & ~1}
    assert _has(r"constexpr int SMALL_WAVES = 16;") and _has(r"constexpr int SMALL_THREADS = SMALL_WAVES \* 64;") and D.SMALL_THREADS == 16 * 64
    assert _has(r"small_kpt\(size_t key_bytes\) \{ return key_bytes <= 4 \? 16 : \(key_bytes == 8 \? 8 : 4\); \}")
    assert D.SMALL_KPT == {1: 16, 2: 16, 4: 16, 8: 8, 16: 4}
    assert _has(rf"constexpr int CHAINS = {D.CHAINS};")
    tiles = {key: K.tile(key) for key in K.KEY_TYPES}
    assert tiles == {"uint8": 16896, "int8": 16896, "uint16": 16896, "int16": 16896, "uint32": 16896, "uint64": 10752, "float64": 7680,
                     "u128": 4608, "i128": 4608}
    assert {K.kpt(key) for key in K.KEY_TYPES} == {22, 14, 10, 6}
    for key in K.KEY_TYPES:
        t, kb = K.tile(key), K.key_bytes(key)
        few, many = K.lengths(key)
        assert few == 3 * t + 1 and many == 37 * t + t // 2 + 3 and many // t >= 4 * D.CHAINS and 0 < many % t < t
        assert few > D.small_tile(kb)                          # above the one-workgroup sort: the pipeline runs
        assert many * kb <= 5_000_000 and many <= 633_603       # far below every route threshold (2^26 keys), and small
    assert set(K.CAN_FAST) == {key for key in K.KEY_TYPES if K.kpt(key) in (22, 10)}


def test_limb_forms_agree_with_big_integers():
    """wide_mapped / wide_order / wide_digits / wide_constant_levels against Python integers"""
    for key in ("u128", "i128"):
        a = H.wide_with_constant_levels(500, key, [3, 7, 8, 15], seed=4)
        a[::5] = a[2]                                           # equal keys: the order is the stable one
        ints = [(int(hi) << 64) | int(lo) for lo, hi in a.tolist()]
        flip = (1 << 127) if key == "i128" else 0
        assert list(H.wide_order(a, key)) == sorted(range(500), key=lambda i: ints[i] ^ flip)
        assert np.array_equal(H.wide_sorted(a, key), a[H.wide_order(a, key)])
        assert K.is_sorted(H.wide_sorted(a, key), key) and not K.is_sorted(a, key)
        m = H.wide_mapped(a, key)
        assert np.array_equal(H.wide_mapped(m, key), a)
        for level in range(16):
            assert H.wide_digits(m, level).tolist() == [((v ^ flip) >> (8 * level)) & 0xFF for v in ints]
        b = H.wide_with_constant_levels(500, key, [3, 7, 8, 15], seed=4)
        assert H.wide_constant_levels(b, key) == {3, 7, 8, 15}
        assert all(set(H.wide_digits(H.wide_mapped(b, key), l).tolist()) == {0x5A} for l in (3, 7, 8, 15))


@pytest.mark.parametrize("key", K.KEY_TYPES)
def test_constant_level_cases_skip_what_they_name(key):
    kb = K.key_bytes(key)
    seen, names = set(), set()
    for name, levels, passes, keys in K.constant_level_cases(key):
        assert len(keys) in K.lengths(key) and (keys.shape == (len(keys), 2) if H.is_wide(key) else keys.dtype == np.dtype(key))
        got = K.constant_levels(keys, key)
        assert got == set(levels), (name, got)
        assert passes == kb - len(got), name
        names.add(name.split(",")[0])
        if passes:
            assert not K.is_sorted(keys, key), name              # not already sorted: the passes run
            seen.add((passes, min(set(range(kb)) - got)))
        else:
            seen.add((0, None))
    assert len(names) == len(K.level_sets(key))
    # odd and even pass counts, a single pass, and (where the width has one) a first executed level above 0
    assert {p % 2 for p, _ in seen} == {0, 1} and 1 in {p for p, _ in seen}
    if kb > 1:
        assert any(f for _p, f in seen if f is not None)
    if kb == 16:
        sets = {frozenset(lv): p for _n, lv, p in K.level_sets(key)}
        assert sets[frozenset(range(1, 16, 2))] == 8 and sets[frozenset({0, 1, 2})] == 13 and sets[frozenset(range(1, 16))] == 1
        assert frozenset({7, 8}) in sets and frozenset(range(8, 16)) in sets and len(sets) == 14
    if kb in (4, 8):
        assert K.level_sets(key) == H.constant_level_sets(kb)


@pytest.mark.parametrize("key", K.COPY_BACK_TYPES)
def test_copy_back_inputs_end_in_tmp_at_every_remainder(key):
    kb = K.key_bytes(key)
    remainders, count = set(), 0
    for keys in K.copy_back_inputs(key):
        got = K.constant_levels(keys, key)
        assert got == K.copy_back_levels(key) and (kb - len(got)) % 2 == 1   # an odd number of passes: the result ends in tmp
        assert not K.is_sorted(keys, key)
        remainders.add(len(keys) * kb % 16)
        count += 1
    assert count == {1: 16, 2: 8, 16: 2}[kb]
    assert remainders == set(range(0, 16, kb))                 # every value the width allows
    places = K.copy_back_placements(key)
    assert places[0][1:] == (0, 0) and all(ko % kb == 0 and to % kb == 0 and 0 <= ko < 16 and 0 <= to < 16 for _n, ko, to in places)
    if kb < 16:
        kinds = {(ko != 0, to != 0) for _n, ko, to in places}
        assert kinds == {(False, False), (True, False), (False, True), (True, True)}
        assert all(ko != to for _n, ko, to in places if ko and to)   # both off by different amounts
    else:
        assert len(places) == 1


def _single_digit_groups(d):
    """for each aligned 64-key group: does it hold one digit"""
    g = d[:len(d) // 64 * 64].reshape(-1, 64)
    return (g == g[:, :1]).all(axis=1)


def _longest_run(d):
    edges = np.flatnonzero(np.diff(d) != 0)
    bounds = np.concatenate(([-1], edges, [len(d) - 1]))
    return int(np.diff(bounds).max())


@pytest.mark.parametrize("key", K.KEY_TYPES)
def test_heavy_digit_inputs_at_key_tile_sizes(key):
    kb = K.key_bytes(key)
    assert K.digit_levels(key) == {1: (0,), 2: (0, 1), 4: (0, 1, 3), 8: (0, 1, 7), 16: (0, 1, 7, 8, 15)}[kb]
    names, levels, sizes = set(), set(), set()
    for name, level, a in K.heavy_digit_cases(key):
        names.add(name)
        levels.add(level)
        sizes.add(len(a))
        d = K.digits(a, key, level)
        if name == "one digit per 64-key round":
            single = _single_digit_groups(d)
            for kpt in (22, 14, 10, 6):                        # every wave span of every keys-only shape holds a single-digit round
                spans = single[:len(single) // kpt * kpt].reshape(-1, kpt)
                assert len(spans) and spans.any(axis=1).all(), (level, len(a), kpt)
        if name == "long equal runs":
            assert _longest_run(d) > 64 * K.kpt(key), (level, len(a))
        if name == "90% one digit":
            assert 0.88 < (d == 0x5A).mean() < 0.92
        if name == "two digits only":
            assert set(np.unique(d)) == {3, 200}
        if name == "sorted by digit":
            assert (np.diff(d) >= 0).all() and len(np.unique(d)) == 256
        if kb > 1:                                              # the other bytes stay random: a misranked round shows as disorder
            other = K.digits(a, key, 0 if level else 1)
            assert len(np.unique(other)) == 256 and not K.is_sorted(a, key)
    assert len(names) == 5 and levels == set(K.digit_levels(key)) and sizes == set(K.lengths(key))


@pytest.mark.parametrize("key", K.CHAIN_SPLIT_TYPES)
def test_chain_split_inputs_are_the_named_shapes(key):
    cases = K.chain_split_inputs(key)
    assert tuple(cases) == K.CHAIN_SPLIT_NAMES
    n = K.lengths(key)[1]
    for name, a in cases.items():
        assert len(a) == (K.short_length(key) if name == "short" else n)
        assert a.shape == (len(a), 2) if H.is_wide(key) else a.dtype == np.dtype(key)
        assert not K.is_sorted(a, key)
    assert D.small_tile(K.key_bytes(key)) < K.short_length(key) < K.tile(key)
    d0 = K.digits(cases["level 0 in one group"], key, 0)
    assert (d0 >> 5 == 0).all() and len(np.unique(d0)) == 32
    d0 = K.digits(cases["level 0 90% in group 7"], key, 0)
    assert 0.9 < (d0 >> 5 == 7).mean() < 0.93 and len(np.unique(d0 >> 5)) == 8
    d1 = K.digits(cases["level 1 only two digits"], key, 1)
    assert set(np.unique(d1)) == {0, 1}
    for name in K.CHAIN_SPLIT_NAMES:                            # every level the shape does not name is busy
        busy = range(1 if name.startswith("level 0") else 0, K.key_bytes(key))
        assert all(len(np.unique(K.digits(cases[name], key, l))) > 1 for l in busy), name


@pytest.mark.parametrize("key", K.DEGENERATE_TYPES)
def test_degenerate_inputs_are_what_they_say(key):
    kb = K.key_bytes(key)
    cases = K.degenerate_inputs(key)
    assert tuple(cases) == K.DEGENERATE_NAMES
    n = K.lengths(key)[1]
    assert all(len(a) == n for a in cases.values())
    rev = cases["reverse sorted"]
    assert K.is_sorted(np.ascontiguousarray(rev[::-1]), key) and not K.is_sorted(rev, key)
    two = cases["two values"]
    assert len(np.unique(two.reshape(n, -1).view(np.uint8).reshape(n, kb), axis=0)) == 2 and not K.is_sorted(two, key)
    one = cases["one level differs"]
    assert K.constant_levels(one, key) == set(range(kb)) - {K.ONE_LEVEL[key]} and not K.is_sorted(one, key)


def test_expected_sorted_is_the_order_of_the_mapped_keys():
    for key in K.KEY_TYPES:
        a = K.random_keys(2000, key, 9)
        a[::3] = a[1]
        e = K.expected_sorted(a, key)
        order = K.order_of(a, key)
        assert K.is_sorted(e, key) and np.array_equal(e.view(np.uint8), a[order].view(np.uint8))
        assert sorted(order.tolist()) == list(range(2000))      # a permutation of the input ...
        same = (K.mapped(a, key)[order][1:] == K.mapped(a, key)[order][:-1]).reshape(1999, -1).all(axis=1)
        assert same.sum() >= 600 and (order[1:][same] > order[:-1][same]).all()   # ... that keeps equal keys in position order
