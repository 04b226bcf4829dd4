"""Inputs shared by tests/test_gpu_segments_nowait.py and tests/test_segments_nowait_inputs.py (no tests here): the tables
and key patterns the tiled route of the nowait segmented sort is held to, and a numpy restatement of its passes — per-tile
digit counts, exclusive prefixes over an item's tiles, digit bases, and the wave-major stable scatter — from which the CPU
test shows that the inputs are what their names say and that the passes, as DESIGN.md §2f states them, sort."""
import numpy as np

from helpers import mapped_key, random_bits
from segments_offsets_inputs import HEAD_GAP, TAIL_GAP, offsets_of

BLOCK_THREADS = 1024             # threads of a tile's workgroup: 16 waves of 64 lanes
WAVES = BLOCK_THREADS // 64
SCAN_CHUNK = 1024                # long items segments_tiles_kernel scans per step
MANY_LONG = 1040                 # long items of the many-items table: more than one chunk, and 2 080 tiles (> 8 x 256)
FLOAT32_SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF,
                             0xFF800001], dtype=np.uint32)   # +-0, +-inf, quiet and signalling NaNs of both signs with payloads


def border_lengths(wave_max, block_max, seed=17):
    """the lengths at which the classes and the tiled route's shapes change (T = block_max), in a seeded shuffle"""
    T = block_max
    lengths = [0, 1, 2, wave_max, wave_max + 1, block_max, block_max + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 17, 5 * T - 1]
    return [int(x) for x in np.random.default_rng(seed).permutation(lengths)]


def long_count(lengths, block_max):
    return int((np.asarray(lengths) > block_max).sum())


def tile_count(lengths, block_max):
    """tiles of the long items: ceil(len / T) each"""
    lengths = np.asarray(lengths, dtype=np.int64)
    long = lengths[lengths > block_max]
    return int((-(-long // block_max)).sum())


def many_items_lengths(wave_max, block_max, seed=23):
    """MANY_LONG long segments of T + 1 ... 2 T keys (both ends occur) mixed with 300 wave-class and 60 block-class ones"""
    rng = np.random.default_rng(seed)
    long = rng.integers(block_max + 1, 2 * block_max + 1, size=MANY_LONG)
    long[:2] = [block_max + 1, 2 * block_max]
    lengths = np.concatenate([long, rng.integers(0, wave_max + 1, size=300), rng.integers(wave_max + 1, block_max + 1, size=60)])
    return [int(x) for x in rng.permutation(lengths)]


def degenerate_tables(wave_max, block_max):
    """(name, offsets, n) of the degenerate tables"""
    T = block_max
    yield ("no long segment",) + offsets_of([0, 5, wave_max, wave_max + 1, block_max, 1, 2, 700])
    yield ("only long segments",) + offsets_of([T + 1, 2 * T + 3, T + 2])
    off = np.array([0, 2 * T + 9], dtype=np.int64)
    yield "one long segment covering the whole array", off, int(off[-1])
    off, n = offsets_of([4, T + 6, 3])
    assert (off[1] % 2) == 1
    yield "a long segment at an odd element index", off, n


def invalid_tables(off, n):
    """(name, offsets, len) of the tables the device must refuse: `off`, a valid table over `n` elements, bent three ways"""
    mid = len(off) // 2
    dec = off.copy()
    dec[mid] = off[mid + 1] + 1
    assert dec[mid + 1] < dec[mid]
    yield "a decreasing pair inside", dec, n
    end = off.copy()
    end[-1] = off[-2] - 1
    assert end[-1] < end[-2]
    yield "a decreasing pair at the end", end, n
    yield "a last offset of len + 1", off, int(off[-1]) - 1


# ---- key patterns of one long segment -----------------------------------------------------------------------------------------

DIGIT_SHAPES = ("all equal", "only byte 2 varies", "strictly descending", "one digit per tile at level 0", "four values")


def digit_shape_keys(shape, n, dtype, T, seed=29):
    """`n` unsigned keys of `dtype` in the named shape; T: the tile"""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    base = random_bits(n, dtype, seed).copy()
    if shape == "all equal":
        base[:] = base[0]
    elif shape == "only byte 2 varies":
        base = (base[0] & ~dt.type(0xFF0000)) | (rng.integers(0, 256, size=n).astype(dt) << dt.type(16))
    elif shape == "strictly descending":
        step = (1 << (8 * dt.itemsize)) // n
        assert step >= 257                      # every level of the keys is busy
        base = (np.arange(n - 1, -1, -1, dtype=np.int64).astype(np.uint64) * np.uint64(step) + rng.integers(0, step, size=n, dtype=np.uint64)).astype(dt)
    elif shape == "one digit per tile at level 0":
        tiles = -(-n // T)
        digits = (np.arange(tiles) * 37 + 11) % 256          # neighbours differ: 37 is odd and below 256
        base = (base & ~dt.type(0xFF)) | np.repeat(digits, T)[:n].astype(dt)
    elif shape == "four values":
        base = base[:4][rng.integers(0, 4, size=n)]
    else:
        raise ValueError(shape)
    return np.ascontiguousarray(base.astype(dt))


def four_value_keys(n, dtype, seed):
    """keys drawn from four values of the type (random bit patterns): every tile is full of ties"""
    pool = random_bits(4, dtype, seed).copy()
    return pool[np.random.default_rng(seed + 1).integers(0, 4, size=n)]


def plant_float32_specials(a, off, seed=31):
    """float32 keys `a` with +-0, +-inf and NaNs of both signs at seeded positions of every segment that can hold them"""
    u = a.view(np.uint32)
    rng = np.random.default_rng(seed)
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        if hi - lo >= 2 * len(FLOAT32_SPECIALS):
            u[lo + rng.choice(hi - lo, size=len(FLOAT32_SPECIALS), replace=False)] = FLOAT32_SPECIALS
    return a


# ---- the tiled passes restated ------------------------------------------------------------------------------------------------

def level_digits(m, level):
    """the digit of every mapped key at `level`"""
    if m.ndim == 2:                     # u128 as (n, 2) uint64 limbs [low, high]
        return ((m[:, level // 8] >> np.uint64(8 * (level % 8))) & np.uint64(0xFF)).astype(np.int64)
    return ((m >> m.dtype.type(8 * level)) & m.dtype.type(0xFF)).astype(np.int64)


def tile_histograms(digits, T):
    """tile_counts as segment_tile_count_kernel writes them: (tiles, 256)"""
    tiles = -(-len(digits) // T)
    tile_of = np.arange(len(digits)) // T
    return np.bincount(tile_of * 256 + digits, minlength=tiles * 256).reshape(tiles, 256)


def tile_offsets(counts):
    """segment_tile_offsets_kernel: per digit the exclusive prefixes over the item's tiles, and the exclusive digit bases"""
    prefix = np.cumsum(counts, axis=0) - counts
    totals = counts.sum(axis=0)
    return prefix, np.cumsum(totals) - totals


def tile_scatter_slots(digits, T, prefix, digit_base):
    """segment_tile_scatter_kernel: the destination of every key of one item.  Inside a tile of n keys, key index =
    wave * 64 * rounds + round * 64 + lane with rounds = ceil(n / 1024); wave w's slots of digit d start at digit_base[d] +
    the tile's prefix + the counts of the waves before it, and inside the wave a key's rank is the number of keys of its
    digit in the rounds before it plus those in the lanes below it (the running slot plus peers_below)."""
    dest = np.empty(len(digits), dtype=np.int64)
    for t in range(prefix.shape[0]):
        d = digits[t * T:(t + 1) * T]
        n = len(d)
        rounds = -(-n // BLOCK_THREADS)
        idx = np.arange(n)
        wave = idx // (64 * rounds)
        per_wave = np.bincount(wave * 256 + d, minlength=WAVES * 256).reshape(WAVES, 256)
        wave_start = digit_base[None, :] + prefix[t][None, :] + np.cumsum(per_wave, axis=0) - per_wave
        group = wave * 256 + d
        order = np.argsort(group, kind="stable")             # (wave, digit) groups, each in (round, lane) order
        sorted_group = group[order]
        first = np.flatnonzero(np.r_[True, sorted_group[1:] != sorted_group[:-1]])
        rank = np.empty(n, dtype=np.int64)
        rank[order] = np.arange(n) - np.repeat(first, np.diff(np.r_[first, n]))
        dest[t * T:t * T + n] = wave_start[wave, d] + rank
    return dest


def tiled_sort_item(keys, T, vals=None):
    """One long item through the route's passes: level by level the counts, the prefixes, the scatter between two arrays, and
    the copy home after an odd number of levels.  Returns (keys, vals) as the route leaves them."""
    m = mapped_key(keys) if keys.ndim == 1 else keys
    levels = keys.dtype.itemsize * (keys.shape[1] if keys.ndim == 2 else 1)
    src_k, src_v = keys, vals
    for level in range(levels):
        digits = level_digits(m, level)
        prefix, base = tile_offsets(tile_histograms(digits, T))
        dest = tile_scatter_slots(digits, T, prefix, base)
        assert np.array_equal(np.sort(dest), np.arange(len(dest))), "the slots are no permutation"
        dst_k, dst_m = np.empty_like(src_k), np.empty_like(m)
        dst_k[dest], dst_m[dest] = src_k, m
        if vals is not None:
            dst_v = np.empty_like(src_v)
            dst_v[dest] = src_v
            src_v = dst_v
        src_k, m = dst_k, dst_m
    return src_k, src_v

