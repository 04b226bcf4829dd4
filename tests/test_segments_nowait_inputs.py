"""CPU checks of tests/segments_nowait_inputs.py: every builder produces the condition it is named for, and the numpy
restatement of the tiled route's passes (counts per tile, prefixes over tiles, digit bases, wave-major stable scatter) sorts
every builder's input — stably, for pairs.  The limits are stated here as rdst_hip_sort_segments_limits gives them and
compared with the library's."""
import numpy as np
import pytest

from helpers import PAIR_WIDTHS, expected_pairs, key_dtype, mapped_key, position_values, random_bits, reference_sorted, same_bits
from segments_nowait_inputs import (DIGIT_SHAPES, FLOAT32_SPECIALS, MANY_LONG, SCAN_CHUNK, border_lengths, degenerate_tables, digit_shape_keys,
                                    four_value_keys, invalid_tables, level_digits, long_count, many_items_lengths, plant_float32_specials,
                                    tile_count, tile_histograms, tile_offsets, tile_scatter_slots, tiled_sort_item)
from segments_offsets_inputs import HEAD_GAP, TAIL_GAP, offsets_of

LIMITS = {(1, 0): (512, 16384), (2, 0): (512, 16384), (4, 0): (512, 16384), (8, 0): (512, 8192), (16, 0): (256, 4096),
          (4, 4): (512, 16384), (4, 8): (512, 8192), (8, 4): (512, 8192), (8, 8): (512, 8192)}
CUS = 256                        # compute units of an MI355X: the many-items table must hold more than 8 tiles per unit


def test_limits_are_the_library_s(hiplib):
    import ctypes
    for (kb, vb), want in LIMITS.items():
        out = (ctypes.c_uint32 * 2)()
        assert hiplib.rdst_hip_sort_segments_limits(kb, vb, out) == 0 and tuple(out) == want, (kb, vb)


def _sorted_u128(a):
    return a[np.lexsort((a[:, 0], a[:, 1]))]


@pytest.mark.parametrize("key", ["uint8", "int16", "uint32", "float32", "int64", "u128"])
def test_border_table_and_the_restatement(key):
    kb = 16 if key == "u128" else np.dtype(key).itemsize
    wave_max, T = LIMITS[(kb, 0)]
    lengths = border_lengths(wave_max, T)
    assert sorted(lengths) == [0, 1, 2, wave_max, wave_max + 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 17, 5 * T - 1]
    assert lengths != sorted(lengths)
    assert long_count(lengths, T) == 6 and tile_count(lengths, T) == 2 + 2 + 2 + 3 + 4 + 5
    off, n = offsets_of(lengths)
    assert off[0] == HEAD_GAP and n - off[-1] == TAIL_GAP
    if key == "u128":
        a = random_bits(2 * n, "uint64", 3).reshape(n, 2).copy()
    else:
        a = random_bits(n, key, 3).copy()
    if key == "float32":
        before = a.copy()
        plant_float32_specials(a, off)
        for s in range(len(off) - 1):
            seg = a[off[s]:off[s + 1]].view(np.uint32)
            assert len(seg) < 2 * len(FLOAT32_SPECIALS) or set(FLOAT32_SPECIALS) <= set(seg), s
        assert not same_bits(a, before)
    for s, length in enumerate(lengths):
        if length <= T:
            continue
        seg = a[off[s]:off[s + 1]]
        got, _ = tiled_sort_item(seg, T)
        want = _sorted_u128(seg) if key == "u128" else reference_sorted(seg)
        assert same_bits(got, want), (key, length)


@pytest.mark.parametrize("dtype", ["uint32", "uint64"])
@pytest.mark.parametrize("shape", DIGIT_SHAPES)
def test_digit_shapes_are_what_they_are_named_for(shape, dtype):
    wave_max, T = LIMITS[(np.dtype(dtype).itemsize, 0)]
    n = 3 * T + 5
    a = digit_shape_keys(shape, n, dtype, T)
    assert a.dtype == np.dtype(dtype) and a.shape == (n,)
    levels = a.dtype.itemsize
    hists = [tile_histograms(level_digits(a, l), T) for l in range(levels)]
    assert all(h.shape == (4, 256) and h.sum() == n for h in hists)
    busy = [int((h.sum(axis=0) > 0).sum()) for h in hists]          # digits in use per level
    if shape == "all equal":
        assert busy == [1] * levels and len(np.unique(a)) == 1       # every level is trivial
    elif shape == "only byte 2 varies":
        assert busy[2] == 256 and all(b == 1 for l, b in enumerate(busy) if l != 2)
    elif shape == "strictly descending":
        assert (a[1:] < a[:-1]).all() and busy[levels - 1] == 256 and busy[0] > 200
    elif shape == "one digit per tile at level 0":
        per_tile = (hists[0] > 0).sum(axis=1)
        assert list(per_tile) == [1, 1, 1, 1]
        digit = hists[0].argmax(axis=1)
        assert (digit[1:] != digit[:-1]).all()
        assert busy[1] == 256                                       # the other bytes stay random
    else:
        assert len(np.unique(a)) == 4 and min(np.unique(a, return_counts=True)[1]) > n // 8
    got, _ = tiled_sort_item(a, T)
    assert same_bits(got, np.sort(a)), shape


@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_restatement_is_stable_for_pairs(kb, vb):
    key = key_dtype(kb, {(4, 4): "u", (4, 8): "i", (8, 4): "f", (8, 8): "u"}[(kb, vb)])
    wave_max, T = LIMITS[(kb, vb)]
    for i, n in enumerate((T + 1, 2 * T, 4 * T + 3)):
        keys = four_value_keys(n, key, 40 + i)
        assert len(np.unique(mapped_key(keys))) == 4
        for t in range(n // T):                                        # every full tile holds all four values: ties throughout
            assert len(np.unique(mapped_key(keys[t * T:(t + 1) * T]))) == 4
        vals = position_values(n, f"uint{8 * vb}")
        gk, gv = tiled_sort_item(keys, T, vals)
        ek, ev = expected_pairs(keys, vals)
        assert same_bits(gk, ek) and same_bits(gv, ev), (kb, vb, n)


def test_scatter_slots_follow_the_wave_major_layout():
    """a tile of 2 049 keys of one digit in three rounds: wave w holds the indices [192 w, 192 w + 192), so the slots are the
    indices themselves; two digits alternate: each digit's keys keep their order"""
    T = 16384
    n = 2049
    d = np.zeros(n, dtype=np.int64)
    prefix, base = tile_offsets(tile_histograms(d, T))
    assert np.array_equal(tile_scatter_slots(d, T, prefix, base), np.arange(n))
    d = np.arange(n) % 2
    prefix, base = tile_offsets(tile_histograms(d, T))
    dest = tile_scatter_slots(d, T, prefix, base)
    assert np.array_equal(dest[d == 0], np.arange(1025)) and np.array_equal(dest[d == 1], 1025 + np.arange(1024))


def test_many_items_table():
    wave_max, T = LIMITS[(2, 0)]
    lengths = many_items_lengths(wave_max, T)
    arr = np.asarray(lengths)
    long = arr[arr > T]
    assert len(long) == MANY_LONG > SCAN_CHUNK                       # the tile scan crosses a chunk
    assert long.min() == T + 1 and long.max() == 2 * T
    assert tile_count(lengths, T) == 2 * MANY_LONG > 8 * CUS         # at least one workgroup takes a second tile
    assert ((arr >= 2) & (arr <= wave_max)).sum() > 100 and ((arr > wave_max) & (arr <= T)).sum() == 60
    # long items lie between batched ones, not in one block
    is_long = arr > T
    assert (is_long[1:] != is_long[:-1]).sum() > 100
    off, n = offsets_of(lengths)
    a = random_bits(n, "uint16", 5)
    picked = [s for s in range(len(lengths)) if lengths[s] > T][::64]   # (the restatement on a sample: all of them take minutes)
    assert len(picked) >= 16
    for s in picked:
        seg = a[off[s]:off[s + 1]]
        got, _ = tiled_sort_item(seg, T)
        assert same_bits(got, np.sort(seg)), s


def test_degenerate_and_invalid_tables():
    wave_max, T = LIMITS[(4, 0)]
    seen = {}
    for name, off, n in degenerate_tables(wave_max, T):
        lengths = np.diff(off)
        assert (lengths >= 0).all() and off[-1] <= n
        seen[name] = (long_count(lengths, T), len(lengths), off, n)
    assert seen["no long segment"][0] == 0 and seen["no long segment"][1] == 8
    assert seen["only long segments"][0] == seen["only long segments"][1] == 3
    one = seen["one long segment covering the whole array"]
    assert one[:2] == (1, 1) and one[2][0] == 0 and one[2][-1] == one[3]
    odd = seen["a long segment at an odd element index"]
    lengths = np.diff(odd[2])
    assert odd[2][int(np.argmax(lengths))] % 2 == 1 and odd[0] == 1
    for with_long in (False, True):
        off, n = offsets_of([3, T + 5 if with_long else 900, 40, 2, 700])
        names = []
        for name, bad, bad_n in invalid_tables(off, n):
            names.append(name)
            decreasing = bool((np.diff(bad) < 0).any())
            assert decreasing or bad[-1] > bad_n, name
            assert decreasing == ("decreasing" in name)
        assert len(names) == 3
