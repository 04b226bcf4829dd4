"""The case lists of tests/devlen_inputs.py are what they claim: the constants are the library's (each found on a line of
rdst_kernels.hip that defines it), every named border is among the lengths of every width, the adversarial tails stand in
the stated relation to their prefixes, and the numpy statement of the result — sort the prefix stably, leave the tail —
equals one stable sort of the whole array under a key that puts the tail above everything in position order."""
import os
import re

import numpy as np
import pytest

import devlen_inputs as D
import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = open(os.path.join(ROOT, "rdst_amd", "csrc", "rdst_kernels.hip")).read()


def _has(pattern):
    return re.search(pattern, SOURCE) is not None


def test_constants_are_the_library_s():
    assert _has(rf"constexpr int HIST_THREADS = {D.HIST_THREADS};")
    assert _has(rf"constexpr int CHAINS = {D.CHAINS};")
    assert _has(r"constexpr int SMALL_WAVES = 16;") and _has(r"constexpr int SMALL_THREADS = SMALL_WAVES \* 64;") and D.SMALL_THREADS == 16 * 64
    assert _has(r"small_kpt\(size_t key_bytes\) \{ return key_bytes <= 4 \? 16 : \(key_bytes == 8 \? 8 : 4\); \}")
    assert D.SMALL_KPT == {1: 16, 2: 16, 4: 16, 8: 8, 16: 4}
    assert _has(r"constexpr uint64_t GRAN = \(uint64_t\)HIST_THREADS \* VEC \* 4;")
    assert _has(rf"constexpr uint32_t ERR_LEN_PAST_CAPACITY = {D.ERR_LEN_PAST_CAPACITY};")
    # the default pass shapes: 12 waves; 22 / 14 / 10 keys per thread for <= 4-byte, unsigned and mapped 8-byte keys; shape 2 for 16
    for row in (r"\{12, 24, 12, 2\},  // 2:", r"\{12, 28, 14, 2\},  // 3:", r"\{12, 22, 11, 1\},  // 4:", r"\{12, 20, 10, 1\},  // 5:"):
        assert _has(row), row
    assert _has(r"if \(elem_bytes == 8\) return mapped \? 5 : 3;") and _has(r"if \(elem_bytes <= 4 && n \* elem_bytes < \(1ull << 32\)\) return 4;")
    assert _has(r"elem_bytes <= 4 \? kpt8 \* 2 : \(elem_bytes == 8 \? kpt8 : \(kpt8 / 2\) & ~1\)")
    assert D.pass_tile(4, False) == 768 * 22 and D.pass_tile(8, False) == 768 * 14 and D.pass_tile(8, True) == 768 * 10 and D.pass_tile(16, False) == 768 * 6
    assert [D.small_tile(b) for b in (1, 2, 4, 8, 16)] == [16384, 16384, 16384, 8192, 4096]
    # the same small tiles as the bounds test quotes
    assert [D.hist_gran(b) for b in (1, 2, 4, 8, 16)] == [65536, 32768, 16384, 8192, 4096]


def test_hist_grid_restated():
    """hist_blocks / hist_piece as the source states them: at most a block per sweep, about sqrt(bytes / 4 KiB) blocks, whole sweeps"""
    assert _has(r"while \(balanced \* balanced \* 4096 < n \* sizeof\(K\)\) \+\+balanced;")
    assert _has(r"uint64_t piece = \(n \+ grid - 1\) / grid;\s+return \(piece \+ gran - 1\) / gran \* gran;")
    for kb in (1, 2, 4, 8, 16):
        g = D.hist_gran(kb)
        assert D.hist_blocks(1, kb) == 1 and D.hist_blocks(g, kb) == 1 and D.hist_blocks(g + 1, kb) == 2
        for n in (2, g + 1, 100_003, 317_000, 10**7):
            b, piece = D.hist_blocks(n, kb), D.hist_piece(n, kb)
            assert 1 <= b <= D.CUS and piece % g == 0 and b * piece >= n and (b - 1) * b * 4096 <= max(n * kb, 4096) * 2
    assert D.hist_blocks(10**9, 4) == D.CUS


def _check_borders(lengths, capacity, tile, key_bytes):
    ms = [m for m, _what in lengths]
    assert ms == sorted(set(ms)) and ms[0] == 0 and ms[-1] == capacity
    g, piece = D.hist_gran(key_bytes), D.hist_piece(capacity, key_bytes)
    want = [0, 1, 2, 3, tile - 1, tile, tile + 1, g - 1, g, g + 1, piece - 1, piece, piece + 1, capacity - 1, capacity]
    for m in want:
        assert m in ms or m > capacity, (m, capacity)
    assert piece < capacity, "the capacity has more than one K1 piece"
    odd = [m for m, what in lengths if what == "odd middle"]
    assert len(odd) == 1 and odd[0] % 2 == 1 and capacity // 4 < odd[0] < 3 * capacity // 4


def test_pair_lengths_hold_every_border():
    assert tuple((kb, vb) for _k, kb, vb in D.PAIR_CASES) == H.PAIR_WIDTHS
    assert {k for k, _kb, _vb in D.PAIR_CASES} == {"u", "i", "f"}
    for _kind, kb, vb in D.PAIR_CASES:
        cap, t = D.pair_capacity(kb, vb), H.pair_tile(kb, vb)
        assert cap == 37 * t + t // 2 + 3 and cap // t >= 4 * D.CHAINS
        lengths = D.pair_lengths(kb, vb)
        _check_borders(lengths, cap, t, kb)
        assert all(m <= cap for m, _ in lengths)     # (a K1 piece may be one sweep long: the two borders then coincide)


def test_key_lengths_hold_every_border():
    widths = [kb for _k, kb in D.KEY_CASES]
    assert sorted(set(widths)) == [1, 2, 4, 8, 16]
    kinds = {np.dtype(k).kind for k, _kb in D.KEY_CASES if k != "u128"}
    assert {"u", "i", "f"} <= kinds
    for key, kb in D.KEY_CASES:
        mapped = key != "u128" and np.dtype(key).kind != "u"
        lengths = D.key_lengths(key, kb)
        _check_borders(lengths, D.KEYS_CAPACITY, D.pass_tile(kb, mapped), kb)   # (one-byte keys: two pieces of one sweep each)
        t = D.small_tile(kb)
        assert D.key_capacities(kb) == (2, 3, t - 1, t, t + 1)
        for cap in D.key_capacities(kb):
            ms = D.small_lengths(cap)
            assert ms[0] == 0 and ms[-1] == cap and all(0 <= m <= cap for m in ms)


@pytest.mark.parametrize("dtype", ("uint32", "int32", "float32", "uint64", "float64"))
def test_tails_stand_in_the_stated_relation(dtype):
    cap, m = 3 * 8448 + 11, 2 * 8448 - 345
    w = np.dtype(dtype).itemsize
    for name in D.TAIL_FAMILIES:
        keys = D.tail_case(name, cap, m, dtype)
        assert keys.dtype == np.dtype(dtype) and len(keys) == cap
        mk = H.mapped_key(keys)
        pre, tail = mk[:m], mk[m:]
        sorted_pre = bool((pre[1:] >= pre[:-1]).all())
        if name == "tail below":
            assert tail.max() < pre.min() and not sorted_pre
        elif name == "tail varies":
            const = [l for l in range(w) if len(np.unique((pre >> np.array(8 * l, dtype=pre.dtype)) & np.array(0xFF, dtype=pre.dtype))) == 1]
            assert const == [1, w - 2]
            for l in const:
                assert len(np.unique((tail >> np.array(8 * l, dtype=tail.dtype)) & np.array(0xFF, dtype=tail.dtype))) > 100
        elif name == "sorted prefix":
            assert sorted_pre and not bool((tail[1:] >= tail[:-1]).all()) and tail.max() < pre.max()
        else:
            inv = np.flatnonzero(mk[1:] < mk[:-1])
            assert list(inv) == [m // 3] and m // 3 + 1 < m
            assert bool((tail[1:] > tail[:-1]).all()) and tail.min() > pre.max()


@pytest.mark.parametrize("key,levels", D.NARROW_WIDE_TAILS, ids=[k for k, _ in D.NARROW_WIDE_TAILS])
def test_narrow_and_wide_tails_stand_in_the_stated_relation(key, levels):
    wide = key == "u128"
    kb = 16 if wide else np.dtype(key).itemsize
    tile = D.pass_tile(kb, not wide and np.dtype(key).kind != "u")
    cap, m = 3 * tile + 11, 2 * tile - 345
    assert D.small_tile(kb) < m < cap                      # (the twin of m keys takes the pipeline as well)
    const = (lambda a: H.wide_constant_levels(a, key)) if wide else H.constant_levels

    def is_sorted(a):
        order = D.order_of(a)
        return bool((order == np.arange(len(a))).all())     # (the stable order of sorted keys is the identity)

    a = D.tail_case_levels("tail varies", cap, m, key, levels)
    assert len(a) == cap and (a.shape == (cap, 2) if wide else a.dtype == np.dtype(key))
    assert const(a[:m]) == set(levels) and (kb - len(levels)) % 2 == 1     # an odd number of passes: the copy-back moves m keys
    assert not const(a[m:]) & set(levels) and not const(a) and not is_sorted(a[:m])
    for l in levels:                                          # the tail varies at the prefix's constant levels: every digit occurs
        d = H.wide_digits(a[m:], l) if wide else (H.mapped_key(a[m:]) >> np.array(8 * l, dtype=f"u{kb}")) & np.array(0xFF, dtype=f"u{kb}")
        assert len(np.unique(d)) == 256

    a = D.tail_case_levels("sorted prefix", cap, m, key, levels)
    assert len(a) == cap and is_sorted(a[:m]) and not is_sorted(a[m:]) and not is_sorted(a)
    assert H.same_bits(D.expected_prefix_sorted(a, m), a)
    last = np.concatenate([a[m - 1:m], a[m:]])               # the prefix's largest key, then the tail: a tail key lies below it
    assert D.order_of(last)[0] != 0


@pytest.mark.parametrize("dtype", ("uint8", "int16", "uint32", "float32", "int64", "float64"))
def test_prefix_sort_is_one_stable_sort_under_the_padded_key(dtype):
    """what a caller of the device-length sort may rely on: sorting the first m elements and leaving the rest equals a stable
    sort of ALL elements whose key is the mapped key below m and, from m on, larger than every key and increasing with the
    position"""
    rng = np.random.default_rng(11)
    for n in (1, 2, 17, 1000):
        keys = H.random_bits(n, dtype, n)
        if n >= 17:
            keys[rng.integers(0, n, size=n // 2)] = keys[0]          # equal keys: stability matters
        vals = H.position_values(n, "uint32")
        for m in sorted({0, 1, n // 3, n - 1, n} & set(range(n + 1))):
            ek, ev = D.expected_prefix_sorted(keys, m, vals)
            order = D.whole_array_order(keys, m)
            assert H.same_bits(ek, keys[order]) and H.same_bits(ev, vals[order])
            assert H.same_bits(ek[m:], keys[m:]) and H.same_bits(ev[m:], vals[m:])
            pk, pv = H.expected_pairs(keys[:m], vals[:m])
            assert H.same_bits(ek[:m], pk) and H.same_bits(ev[:m], pv)
    # the 128-bit container: rows of limbs [low, high], ordered by the high limb first
    limbs = np.array([[5, 1], [0, 2], [9, 0], [1, 1]], dtype=np.uint64)
    assert list(D.order_of(limbs)) == [2, 3, 0, 1]
    assert np.array_equal(D.expected_prefix_sorted(limbs, 3), limbs[[2, 0, 1, 3]])
