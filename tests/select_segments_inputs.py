"""Inputs and numpy statements for the segmented select (rdst_hip_select_segments_device): the rank rule
restated with fractions.Fraction, THE result — per segment the elements of a stable argsort by the mapped key at the ranks
the specs stand for in a segment of that length —, the stream class's select restated (levels until m <= TILE: the keys before
the prefix are only counted) and the case tables of tests/test_gpu_select_segments.py.

A spec is a tuple (num, den, mode): den == 0 is the absolute rank num; otherwise the quantile num / den rounded by mode
(0 lower, 1 higher, 2 nearest, half to even).  Keys are 1-D numpy arrays of a built-in dtype, or (n, 2) uint64 rows of limbs
with key="u128" / "i128"; offsets count keys."""
import functools
from fractions import Fraction

import numpy as np

import helpers as H
import topk_inputs as T
import topk_segments_inputs as S

LOWER, HIGHER, NEAREST = 0, 1, 2
MODES = {"lower": LOWER, "higher": HIGHER, "nearest": NEAREST}
MAX_RANKS = 32                                                              # specs per round (rdst_segments_layout.h)


def limits(kb, indexed, stream_max=0):
    """(wave_max, block_max, stream_max, max_ranks): the plan's classes at k = 1, so a segment's class follows from its length"""
    wm, bm, sm, _ksm = S.limits(kb, indexed, stream_max)
    return wm, bm, sm, MAX_RANKS


def spec_ok(spec):
    num, den, mode = spec
    if not (0 <= num < 1 << 32 and 0 <= den < 1 << 32 and 0 <= mode <= 2):
        return False
    return mode == 0 if den == 0 else num <= den


@functools.lru_cache(maxsize=None)
def rank_of(spec, n):
    """the rank `spec` stands for in a segment of n keys, or None: the rule in exact rationals"""
    num, den, mode = spec
    if n == 0:
        return None
    if den == 0:
        return num if num < n else None
    v = Fraction((n - 1) * num, den)                                        # numpy's virtual index for these three methods
    floor = v.numerator // v.denominator
    if mode == LOWER or v == floor:
        return floor
    if mode == HIGHER:
        return floor + 1
    frac = v - floor
    if frac != Fraction(1, 2):
        return floor + (1 if frac > Fraction(1, 2) else 0)
    return floor + (floor & 1)                                              # half way: to the even neighbour


def expected_rows(a, offsets, specs, largest, key, out_keys, out_index=None, ordered=None):
    """THE result of a whole table, written into the pre-filled (n_segments, n_ranks[, 2]) array `out_keys` (and the
    (n_segments, n_ranks) integer array `out_index`): slot i of row s is element rank_of(specs[i], n_s) of segment s's stable
    order; a slot without a rank keeps what it holds.  `ordered`: topk_segments_inputs.table_order's answer, if the caller has
    it (one stable sort by (segment, mapped key): segment s occupies the sorted places [offsets[s] - offsets[0], ...))."""
    off = np.asarray(offsets, dtype=np.int64)
    order, _sseg, _rank = ordered if ordered is not None else S.table_order(a, offsets, largest, key)
    lens = off[1:] - off[:-1]
    body = a[int(off[0]):int(off[-1])]
    for i, spec in enumerate(specs):
        r = [rank_of(tuple(spec), int(n)) for n in lens]
        rows = np.array([s for s, v in enumerate(r) if v is not None], dtype=np.int64)
        if rows.size == 0:
            continue
        at = order[(off[rows] - off[0]) + np.array([v for v in r if v is not None], dtype=np.int64)]
        out_keys[rows, i] = body[at]
        if out_index is not None:
            out_index[rows, i] = at - (off[rows] - off[0])


def stream_select(seg, r, largest, tile, key=None):
    """The stream class's select for rank r of one segment: a digit per level, most significant first, over the keys still on
    the prefix, until m <= tile or the digits are exhausted.  Returns (levels, c_below, m): the stage then holds the ranks
    [c_below, c_below + m) — or, with m > tile (all keys on the prefix equal), a window of them."""
    name = key if key else seg.dtype.name
    kb = T.key_bytes(name)
    hi, lo = T.mapped_limbs(seg, name, largest)
    if not T.is_wide(name) and kb < 8 and largest:
        lo = lo & np.uint64((1 << (8 * kb)) - 1)                            # the complement inside the key's width
    on = np.ones(len(seg), dtype=bool)
    levels, c_below, m = 0, 0, len(seg)
    for _pos, shift, bits in T.level_shapes(kb, False):
        if m <= tile:
            break
        d = T._digit(hi, lo, kb, shift, bits)
        counts = np.bincount(d[on], minlength=1 << bits)
        cum = np.cumsum(counts)
        b = int(np.searchsorted(cum, r + 1 - c_below, side="left"))
        c_below += int(cum[b] - counts[b])
        m = int(counts[b])
        on &= d == b
        levels += 1
    return levels, c_below, m


def descents(seg, ranks, largest, tile, key=None):
    """how many times the stream class runs its select for these resolved ranks: they are served in ascending order, and a rank
    inside what the stage holds costs nothing (m > tile: the window of `tile` ordinals)"""
    count, lo, filled = 0, 0, 0
    for r in sorted(ranks):
        if lo <= r < lo + filled:
            continue
        _levels, c_below, m = stream_select(seg, r, largest, tile, key)
        first = (r - c_below) // tile * tile if m > tile else 0
        lo, filled = c_below + first, min(tile, m - first)
        count += 1
    return count


# ---- case tables -----------------------------------------------------------------------------------------------------------

def median(mode=LOWER):
    return (1, 2, mode)


def rank_sets(wm):
    """the rank sets of the length tables: absolute 0, the lower median, the quantile 1/1, and a mixed set of five with a repeat
    and an absolute rank (wave_max) that the short segments lack — the absolute rank first and one mode, as the Python
    wrapper passes them (tests/cpp/test_rdst_select_segments.cpp mixes the modes in one call)"""
    return [[(0, 0, 0)], [median()], [(1, 1, LOWER)], [(wm, 0, 0), (9, 10, NEAREST), median(NEAREST), (9, 10, NEAREST), (1, 3, NEAREST)]]


def many_specs(count, seed):
    """`count` specs: quantiles k / (count - 1) in shuffled order and all three modes, with absolute ranks among them"""
    rng = np.random.default_rng(seed)
    specs = [(k, count - 1, int(rng.integers(0, 3))) for k in range(count)]
    for at, r in ((3, 0), (count // 2, 700), (count - 2, 40000)):
        specs[at] = (r, 0, 0)
    return [specs[i] for i in rng.permutation(count)]


def prefix_border(dtype, tile, n, extra, seed):
    """n keys (n > tile) and a rank r: after ONE level of the ascending select exactly tile + extra keys lie on r's prefix.
    Top digit 1 for `below` keys, 2 for tile + extra keys (r is among them), 3 for the rest; random below the digit.  With
    more keys before the prefix than the partial sort's stop rule (c_below + m <= tile) would allow.  Returns (keys, r)."""
    rng = np.random.default_rng(seed)
    kb = np.dtype(dtype).itemsize
    w = 8 * kb
    m = tile + extra
    below = (n - m) // 2
    digit = np.full(n, 3, dtype=np.uint64)
    at = rng.permutation(n)
    digit[at[:below]] = 1
    digit[at[below:below + m]] = 2
    low = rng.integers(0, 1 << (w - 12), size=n, dtype=np.uint64)
    keys = H.unmapped(((digit << np.uint64(w - 12)) | low).astype(f"u{kb}"), dtype)
    return keys, below + m // 2


def window_ranks(tile):
    """ranks in the windows 0, 1, 2 and 3 of an all-equal segment of 3 tile + 5 keys (two of them share window 1)"""
    return [5, tile + 7, 2 * tile + 1, 3 * tile + 4, 2 * tile - 1]


def float_zero_nan_segment(dtype, n, seed):
    """n floats: a third ordinary values, then runs of -0.0, +0.0 and NaNs of both signs with two payloads each, shuffled.
    Returns (keys, ranks): the first and last rank of every special run in the ascending order."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    w = 8 * dt.itemsize
    u = np.dtype(f"u{dt.itemsize}")
    mant = 23 if w == 32 else 52
    sign, quiet = 1 << (w - 1), ((1 << (w - 1)) - 1) ^ ((1 << (mant - 1)) - 1)   # a NaN: exponent all ones and the top mantissa bit
    specials = [sign, 0, quiet | 1, quiet | 2, sign | quiet | 1, sign | quiet | 2]
    a = T.random_keys(n, dtype, seed).view(u)
    per = n // 9
    for i, bits in enumerate(specials):
        a[n // 3 + i * per:n // 3 + (i + 1) * per] = bits
    a = a[rng.permutation(n)].view(dt)
    m = np.sort(H.mapped_key(a))
    ranks = []
    for bits in specials:
        key = H.mapped_key(np.array([bits], dtype=u).view(dt))[0]
        ranks += [int(np.searchsorted(m, key, side="left")), int(np.searchsorted(m, key, side="right")) - 1]
    return a, ranks
