"""Inputs of the keys-only tests at every key width (tests/test_gpu_keys.py): the whole-slice scatter pipeline — K1, K2, K3 and
the copy-back — under 1-, 2- and 16-byte keys and unsigned 8-byte keys, each a pass shape of its own, with one 4-byte and one
float 8-byte type beside them for comparison.  Skipped levels at both parities of the passes left, an odd number of passes
between guard bands, heavy digits, chain-split shapes and degenerate orders.  16-byte keys are (n, 2) uint64 rows of limbs
[low, high].  Shared by the CPU test of the inputs (tests/test_keys_inputs.py) and the GPU test, so that both see the same
cases."""
import numpy as np

import devlen_inputs as D
import helpers as H

KEY_TYPES = ("uint8", "int8", "uint16", "int16", "uint32", "uint64", "float64", "u128", "i128")
CAN_FAST = ("uint8", "int8", "uint16", "int16", "uint32", "float64")   # pass shapes 4 and 5: the returning-add ranking


def key_bytes(key):
    return 16 if H.is_wide(key) else np.dtype(key).itemsize


def is_mapped(key):
    """does the key map change bits (the 8-byte pass shape depends on it)"""
    return key == "i128" or (not H.is_wide(key) and np.dtype(key).kind != "u")


def kpt(key):
    return D.PASS_KPT[(key_bytes(key), is_mapped(key))]


def tile(key):
    """keys per tile of the type's default pass shape"""
    return D.PASS_THREADS * kpt(key)


def lengths(key):
    """a few tiles with a single key in the last one; several tiles on every one of the 8 chains and a partial last tile"""
    t = tile(key)
    return 3 * t + 1, 37 * t + t // 2 + 3


def uint_name(key):
    return f"uint{8 * key_bytes(key)}"


def from_mapped(m, key):
    """the keys of type `key` whose mapped images are `m` (an unsigned array, or rows of mapped limbs)"""
    return H.wide_mapped(m, key) if H.is_wide(key) else H.unmapped(m, key)


def mapped(a, key):
    return H.wide_mapped(a, key) if H.is_wide(key) else H.mapped_key(a)


def digits(a, key, level):
    """the mapped digit of every key at `level`"""
    m = mapped(a, key)
    if H.is_wide(key):
        return H.wide_digits(m, level)
    return ((m >> np.array(8 * level, dtype=m.dtype)) & np.array(0xFF, dtype=m.dtype)).astype(np.int64)


def constant_levels(a, key):
    return H.wide_constant_levels(a, key) if H.is_wide(key) else H.constant_levels(a)


def order_of(a, key):
    return H.wide_order(a, key) if H.is_wide(key) else np.argsort(H.mapped_key(a), kind="stable")


def expected_sorted(a, key):
    """THE result: helpers.reference_sorted; rows of limbs by np.lexsort((low, high)) of the mapped limbs"""
    return H.wide_sorted(a, key) if H.is_wide(key) else H.reference_sorted(a)


def is_sorted(a, key):
    m = mapped(a, key)
    if H.is_wide(key):
        hi, lo = m[:, 1], m[:, 0]
        return bool(((hi[1:] > hi[:-1]) | ((hi[1:] == hi[:-1]) & (lo[1:] >= lo[:-1]))).all())
    return bool((m[1:] >= m[:-1]).all())


def random_keys(n, key, seed):
    if H.is_wide(key):
        return np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 2), dtype=np.uint64, endpoint=False)
    return H.random_bits(n, key, seed).copy()


def with_constant_levels(n, key, levels, seed):
    if H.is_wide(key):
        return H.wide_with_constant_levels(n, key, sorted(levels), seed)
    return H.keys_with_constant_levels(n, key, sorted(levels), seed)


# ---- 1: skipped levels, both pass parities ----------------------------------------------------------------------------------

def level_sets(key):
    """(name, constant levels, passes left) of the skipped-level cases of a key type"""
    kb = key_bytes(key)
    every = set(range(kb))
    if kb == 1:
        sets = [("none", set()), ("all", every)]
    elif kb == 2:
        sets = [("level 0", {0}), ("level 1", {1}), ("none", set())]
    elif kb in (4, 8):
        return H.constant_level_sets(kb)
    else:
        sets = [("level 0", {0}), ("level 1", {1}), ("level 15", {15}), ("level 7", {7}), ("level 8", {8}),
                ("levels 7 and 8", {7, 8}),                     # both sides of the limb border
                ("levels 0 and 1", {0, 1}), ("all but level 0", every - {0}), ("all but level 15", every - {15}),
                ("all but level 8", every - {8}),
                ("every odd level", set(range(1, 16, 2))),       # eight passes, a skip between every two that run
                ("levels 8 to 15", set(range(8, 16))),           # only the low limb varies
                ("levels 0 to 2", {0, 1, 2}),                    # thirteen passes
                ("none", set())]
    return [(f"{name} constant", levels, kb - len(levels)) for name, levels in sets]


def constant_level_cases(key):
    """(name, levels, passes, keys) of every skipped-level case, at both lengths"""
    for j, n in enumerate(lengths(key)):
        for i, (name, levels, passes) in enumerate(level_sets(key)):
            yield f"{name}, n={n}", levels, passes, with_constant_levels(n, key, levels, seed=7000 + 100 * j + i)


# ---- 2: the copy-back moving data --------------------------------------------------------------------------------------------
COPY_BACK_TYPES = ("uint8", "int8", "uint16", "int16", "u128", "i128")
COPY_BACK_BAND = 4096


def copy_back_levels(key):
    """the constant levels of the copy-back inputs: an odd number of passes is left — 1, 1 and 13"""
    return {1: set(), 2: {1}, 16: {0, 1, 2}}[key_bytes(key)]


def copy_back_inputs(key):
    """consecutive lengths from the short one — 16, 8 and 2 of them — so that n * sizeof(K) leaves every remainder modulo 16
    the width allows: the vector body and the tail of copyback_body both carry data"""
    kb = key_bytes(key)
    n0 = lengths(key)[0]
    for r in range({1: 16, 2: 8, 16: 2}[kb]):
        yield with_constant_levels(n0 + r, key, copy_back_levels(key), seed=7500 + r)


def copy_back_placements(key):
    """(name, byte offset of keys, of tmp) from a 16-byte boundary; 16-byte keys: the entry takes aligned buffers only"""
    kb = key_bytes(key)
    if kb == 16:
        return [("both aligned", 0, 0)]
    return [("both aligned", 0, 0), (f"only keys at +{3 * kb}", 3 * kb, 0), (f"only tmp at +{5 * kb}", 0, 5 * kb),
            (f"keys at +{kb}, tmp at +{7 * kb}", kb, 7 * kb)]


# ---- 3: heavy digits ------------------------------------------------------------------------------------------------------------

def digit_levels(key):
    kb = key_bytes(key)
    return {1: (0,), 2: (0, 1), 4: (0, 1, 3), 8: (0, 1, 7), 16: (0, 1, 7, 8, 15)}[kb]


def long_run(key):
    """the run length of "long equal runs": longer than the keys one wave takes from a tile (64 * KPT), so that a wave's
    whole span holds one digit"""
    return max(1000, 96 * kpt(key))


def heavy_digit_cases(key):
    """(name, level, keys) of helpers.heavy_digit_inputs at both lengths and every level of digit_levels, the digit shapes
    built on the MAPPED key (a float's raw byte is complemented under the negatives); the lower bytes stay random"""
    for n in lengths(key):
        for level in digit_levels(key):
            if H.is_wide(key):
                cases = H.wide_heavy_digit_inputs(n, key, level, seed=n + level, run=long_run(key))
            else:
                cases = {name: H.unmapped(m, key)
                         for name, m in H.heavy_digit_inputs(n, uint_name(key), level, seed=n + level, run=long_run(key)).items()}
            for name, a in cases.items():
                yield name, level, a


# ---- 4: chain split --------------------------------------------------------------------------------------------------------------
CHAIN_SPLIT_TYPES = ("uint16", "u128")
CHAIN_SPLIT_NAMES = ("level 0 in one group", "level 0 90% in group 7", "level 1 only two digits", "short")


def short_length(key):
    """a slice shorter than a tile that still takes the pipeline (longer than the one-workgroup sort's tile)"""
    n = tile(key) - 5
    assert n > D.small_tile(key_bytes(key))
    return n


def chain_split_inputs(key):
    """the cases of helpers.chain_split_cases that make sense at the width, at the long length: the shapes live in the two
    lowest bytes, which a 2-byte key keeps whole and a 16-byte key carries in its low limb (the high limb is random)"""
    n = lengths(key)[1]
    cases = H.chain_split_cases(n, "uint64", seed=77 + key_bytes(key), short=short_length(key))
    out = {}
    for name in CHAIN_SPLIT_NAMES:
        low = np.ascontiguousarray(cases[name])
        if H.is_wide(key):
            high = np.random.default_rng(78).integers(0, 1 << 64, size=len(low), dtype=np.uint64, endpoint=False)
            out[name] = np.stack([low, high], axis=1)
        else:
            out[name] = low.astype(np.dtype(key))                # (the low bytes)
    return out


# ---- 5: degenerate orders ------------------------------------------------------------------------------------------------------
DEGENERATE_TYPES = ("uint8", "int16", "u128", "i128")
DEGENERATE_NAMES = ("reverse sorted", "two values", "one level differs")
ONE_LEVEL = {"uint8": 0, "int16": 1, "u128": 3, "i128": 15}   # the level that differs (int16, i128: the one with the sign)


def degenerate_inputs(key):
    n = lengths(key)[1]
    base = random_keys(n, key, 5100)
    rev = np.ascontiguousarray(expected_sorted(base, key)[::-1])
    pool = random_keys(2, key, 5101)
    two = pool[np.random.default_rng(5102).integers(0, 2, size=n)]
    one = with_constant_levels(n, key, set(range(key_bytes(key))) - {ONE_LEVEL[key]}, seed=5103)
    return {"reverse sorted": rev, "two values": two, "one level differs": one}
