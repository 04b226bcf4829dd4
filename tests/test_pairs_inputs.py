"""The inputs of tests/test_gpu_pairs.py, checked where no device is needed: each case provably is what its name says (the
levels a sort skips and the parity of the passes left, single-digit rounds and long runs at pair tile sizes), the values name
their positions, and the reference is the stable order."""
import numpy as np
import pytest

from helpers import (COPY_BACK_LEVELS, PAIR_KPT, PAIR_WIDTHS, constant_level_inputs, constant_level_sets, constant_levels, copy_back_inputs,
                     expected_pairs, mapped_key, pair_heavy_digit_inputs, pair_kpt, pair_lengths, pair_tile, position_values, value_positions)


def test_pair_tiles():
    assert [pair_tile(kb, vb) for kb, vb in PAIR_WIDTHS] == [8448, 5376, 5376, 3840]
    for kb, vb in PAIR_WIDTHS:
        t = pair_tile(kb, vb)
        few, many = pair_lengths(kb, vb)
        assert few % t == 1 and few // t == 3
        assert many // t >= 8 * 4 and 0 < many % t < t and many <= 320_000


@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
@pytest.mark.parametrize("kind", ["u", "i", "f"])
def test_constant_level_cases_skip_what_they_name(kb, vb, kind):
    seen = set()
    for name, levels, passes, keys in constant_level_inputs(kb, vb, kind):
        assert len(keys) in pair_lengths(kb, vb)
        got = constant_levels(keys)
        assert got == set(levels), (name, got)
        assert passes == kb - len(got), name
        m = mapped_key(keys)
        assert (m[1:] < m[:-1]).any(), name      # not already sorted: the passes run
        if name.startswith("one sign"):
            assert kind == "f" and not np.signbit(keys).any() and len(np.unique(m >> np.array(8 * kb - 8, dtype=m.dtype))) > 64
        seen.add((passes, min(set(range(kb)) - got)))
    # odd and even pass counts, a first executed level of 0 and higher ones, a single pass
    assert {p % 2 for p, _ in seen} == {0, 1} and {f for _, f in seen} >= {0, 1, 2} and 1 in {p for p, _ in seen}


def test_constant_level_sets_hold_a_skip_between_two_executed_levels():
    for kb in (4, 8):
        sets = [lv for _name, lv, _passes in constant_level_sets(kb)]
        assert any(l - 1 not in lv and l + 1 not in lv and 0 < l < kb - 1 for lv in sets for l in lv)
        assert set() in sets


@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_copy_back_inputs_end_in_tmp_at_every_remainder(kb, vb):
    """every length of the copy-back tests keeps level 1 (and only it) constant: an odd number of passes, so both
    copyback_kernel launches move data; and the lengths leave every remainder of n * sizeof(V) modulo 16"""
    remainders = set()
    for keys in copy_back_inputs(kb, vb):
        assert constant_levels(keys) == COPY_BACK_LEVELS and (kb - len(COPY_BACK_LEVELS)) % 2 == 1
        m = mapped_key(keys)
        assert (m[1:] < m[:-1]).any()
        remainders.add(len(keys) * vb % 16)
    assert remainders == ({0, 4, 8, 12} if vb == 4 else {0, 8})
    assert {len(k) * kb % 16 for k in copy_back_inputs(kb, vb)} == ({0, 4, 8, 12} if kb == 4 else {0, 8})


def _single_digit_groups(d):
    """for each aligned 64-key group: does it hold one digit"""
    g = d[:len(d) // 64 * 64].reshape(-1, 64)
    return (g == g[:, :1]).all(axis=1)


def _longest_run(d):
    edges = np.flatnonzero(np.diff(d) != 0)
    bounds = np.concatenate(([-1], edges, [len(d) - 1]))
    return int(np.diff(bounds).max())


@pytest.mark.parametrize("kb,vb", PAIR_WIDTHS)
def test_heavy_digit_inputs_at_pair_sizes(kb, vb):
    names = set()
    for name, level, a in pair_heavy_digit_inputs(kb, vb):
        names.add(name)
        d = ((mapped_key(a) >> np.array(8 * level, dtype=f"u{kb}")) & np.array(0xFF, dtype=f"u{kb}")).astype(np.int64)
        if name == "one digit per 64-key round":
            single = _single_digit_groups(d)
            for kpt in sorted(set(PAIR_KPT.values())):            # 5, 7 and 11: every wave span holds a single-digit round
                spans = single[:len(single) // kpt * kpt].reshape(-1, kpt)
                assert len(spans) and spans.any(axis=1).all(), (level, len(a), kpt)
        if name == "long equal runs":
            assert _longest_run(d) > 64 * max(PAIR_KPT.values()), (level, len(a))
    assert len(names) == 5 and pair_kpt(kb, vb) in (5, 7, 11)


@pytest.mark.parametrize("vdtype", ["int32", "int64"])
def test_position_values_name_their_positions(vdtype):
    lengths = sorted({n for kb, vb in PAIR_WIDTHS for n in pair_lengths(kb, vb)} | {2, 700, 8400})
    for n in lengths:
        v = position_values(n, vdtype)
        assert v.dtype == np.dtype(vdtype) and len(np.unique(v)) == n
        assert np.array_equal(value_positions(v), np.arange(n))
    v = position_values(lengths[-1], vdtype)
    w = 8 * v.dtype.itemsize
    bits = np.bitwise_or.reduce(v.view(f"u{w // 8}")), np.bitwise_and.reduce(v.view(f"u{w // 8}"))
    assert int(bits[0]) == (1 << w) - 1 and int(bits[1]) == 0     # every bit of the value takes both values


def test_expected_pairs_is_the_stable_order():
    rng = np.random.default_rng(5)
    for dtype in ("uint32", "int64", "float32"):
        pool = rng.integers(0, 1 << 32, size=40, dtype=np.uint64).astype(f"u{np.dtype(dtype).itemsize}").view(dtype)
        keys = pool[rng.integers(0, 40, size=1000)].copy()
        vals = position_values(1000, "int64")
        mk = mapped_key(keys).tolist()
        order = sorted(range(1000), key=lambda i: mk[i])          # Python's sort is stable
        ek, ev = expected_pairs(keys, vals)
        assert ek.view(f"u{keys.dtype.itemsize}").tolist() == keys[order].view(f"u{keys.dtype.itemsize}").tolist()
        assert ev.tolist() == vals[order].tolist()
        assert len(set(mk)) < 1000
