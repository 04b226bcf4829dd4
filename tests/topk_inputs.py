"""Inputs and numpy statements for the partial sort (rdst_hip_topk_device): the case lists of
tests/test_gpu_topk.py, THE result as a stable argsort over helpers.mapped_key, and the select's level loop restated, so
that a test can say which depth a case reaches and compare it with what the device reports (rdst_hip_debug_topk_state).

Keys are 1-D numpy arrays of a built-in dtype, or (n, 2) uint64 rows of limbs [low, high] with key="u128" / "i128"."""
import numpy as np

import helpers as H

# the library's constants, quoted from rdst_amd/csrc/rdst_topk.hip and rdst_topk_layout.h (tests/test_topk_inputs.py looks each of them up)
COUNTERS = 4096
DIGIT_BITS_WIDE = 12
DIGIT_BITS_BYTE = 8
POSITION_BITS = 32
DEFAULT_CAND_CAPACITY = 1 << 20
HIST_THREADS = 256
HIST_UNROLL = 4
BLOCKS_PER_CU = 8
CUS = 256                        # compute units of the one device the library is built for

# every key type keys-only: (name, key bytes); "u128" / "i128" are rows of limbs
KEY_TYPES = (("uint8", 1), ("uint16", 2), ("uint32", 4), ("uint64", 8), ("u128", 16), ("int8", 1), ("int16", 2), ("int32", 4), ("int64", 8),
             ("i128", 16), ("float32", 4), ("float64", 8))
# with an index: 4- and 8-byte keys, both index widths
INDEX_CASES = (("uint32", 4), ("int32", 8), ("float32", 4), ("uint64", 8), ("int64", 4), ("float64", 8))
KS = (1, 2, 63, 64, 65, -1, 0)   # -1: len - 1, 0: len


def is_wide(key):
    return key in ("u128", "i128")


def key_bytes(key):
    return 16 if is_wide(key) else np.dtype(key).itemsize


def digit_bits(kb):
    return DIGIT_BITS_BYTE if kb == 1 else DIGIT_BITS_WIDE


def key_levels(kb):
    return -(-8 * kb // digit_bits(kb))


def max_levels(kb, indexed):
    return key_levels(kb) + (-(-POSITION_BITS // digit_bits(kb)) if indexed else 0)


def level_shapes(kb, indexed):
    """(is a position level, shift, bits) of every level a call can take, most significant first; the last level of a
    field is the narrow one"""
    d = digit_bits(kb)
    out = []
    for pos, bits in ((False, 8 * kb), (True, POSITION_BITS))[:2 if indexed else 1]:
        hi = bits
        while hi > 0:
            lo = max(hi - d, 0)
            out.append((pos, lo, hi - lo))
            hi = lo
    return out


def vec(kb):
    """keys per 16-byte load"""
    return 16 // kb


def block_batch(kb):
    """keys one workgroup of the streaming kernels takes per trip of its loop"""
    return HIST_THREADS * vec(kb) * HIST_UNROLL


def grid_worth(kb, cus=CUS):
    """keys one trip of the whole grid covers on a device of `cus` compute units (the GPU test asks the device)"""
    return cus * BLOCKS_PER_CU * block_batch(kb)


def border_lengths(kb):
    """the short lengths at which the streaming kernels change what they do"""
    b = block_batch(kb)
    return sorted({1, 2, max(vec(kb) - 1, 1), vec(kb), vec(kb) + 1, b - 1, b, b + 1, HIST_THREADS * vec(kb) + 1})


def ks_for(n):
    return sorted({k if k > 0 else n + k for k in KS if (k if k > 0 else n + k) >= 1 and (k if k > 0 else n + k) <= n})


def random_keys(n, key, seed):
    if is_wide(key):
        return np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 2), dtype=np.uint64, endpoint=False)
    return H.random_bits(n, key, seed).copy()


def mapped_limbs(a, key, largest=False):
    """(high, low) uint64 limbs of the mapped key (complemented for largest); a key of up to 8 bytes sits in `low`, in its
    own width, and `high` is 0"""
    if is_wide(key):
        lo, hi = a[:, 0].copy(), a[:, 1].copy()
        if key == "i128":
            hi ^= np.uint64(1 << 63)
        if largest:
            lo, hi = ~lo, ~hi
        return hi, lo
    m = H.mapped_key(a)
    if largest:
        m = ~m
    return np.zeros(len(a), dtype=np.uint64), m.astype(np.uint64)


def order_of(a, key=None, largest=False):
    """the stable order by the mapped key (largest: by its complement — equal keys still in ascending position)"""
    if is_wide(key):
        hi, lo = mapped_limbs(a, key, largest)
        return np.lexsort((lo, hi))
    m = H.mapped_key(a)
    return np.argsort(~m if largest else m, kind="stable")


def expected_topk(a, k, largest=False, key=None):
    """THE result: (keys, positions) of the first k elements of a stable argsort by the mapped key (complemented for
    largest)"""
    order = order_of(a, key, largest)[:k]
    return a[order], order.astype(np.int64)


def _digit(hi, lo, kb, shift, bits):
    """bits [shift, shift + bits) of the (high, low) limbs of a key of kb bytes"""
    mask = np.uint64((1 << bits) - 1)
    if shift >= 64:
        return ((hi >> np.uint64(shift - 64)) & mask).astype(np.int64)
    d = lo >> np.uint64(shift)
    if shift + bits > 64:
        d = d | (hi << np.uint64(64 - shift))
    return (d & mask).astype(np.int64)


def restate(a, k, largest=False, indexed=False, cand_capacity=0, key=None):
    """The select's level loop as the device runs it: counts of the next digit over the elements still on the prefix, the
    bucket of the (k - c_below)-th, until the bucket holds at most cand_capacity elements or the digits are exhausted.
    Returns what rdst_hip_debug_topk_state reports — levels, c_below, candidates, special — and `m`, the bucket's size."""
    kb = key_bytes(key if key else a.dtype.name)
    n = len(a)
    cap = min(cand_capacity or DEFAULT_CAND_CAPACITY, max(n, 1))
    hi, lo = mapped_limbs(a, key if key else a.dtype.name, largest)
    pos = np.arange(n, dtype=np.uint64)
    on = np.ones(n, dtype=bool)
    levels, c_below, m, special, fill = 0, 0, n, 0, False
    shapes = level_shapes(kb, indexed)
    if n > cap:
        for i, (is_pos, shift, bits) in enumerate(shapes):
            d = _digit(np.zeros(n, dtype=np.uint64), pos, 8, shift, bits) if is_pos else _digit(hi, lo, kb, shift, bits)
            counts = np.bincount(d[on], minlength=1 << bits)
            cum = np.cumsum(counts)
            remaining = k - c_below
            b = int(np.searchsorted(cum, remaining, side="left"))
            c_below += int(cum[b] - counts[b])
            m = int(counts[b])
            on &= d == b
            levels = i + 1
            special |= int(is_pos)
            last = i + 1 == len(shapes)
            if last and m > cap:
                fill, special = True, 1
            if last or m <= cap:
                break
    return {"levels": levels, "c_below": c_below, "candidates": 0 if fill else m, "special": special, "m": m}


def direct_depth(a, k, largest, indexed, cand_capacity):
    """The depth stated without the loop (keys of up to 8 bytes): the fewest leading levels whose digits, taken from the
    k-th element of the stable order, are shared by at most cand_capacity elements."""
    kb = a.dtype.itemsize
    n = len(a)
    cap = min(cand_capacity or DEFAULT_CAND_CAPACITY, max(n, 1))
    m = H.mapped_key(a).astype(np.uint64)
    if largest:
        m = (~m) & np.uint64((1 << (8 * kb)) - 1) if kb < 8 else ~m
    t = int(order_of(a, None, largest)[k - 1])
    same = np.ones(n, dtype=bool)
    shapes = level_shapes(kb, indexed)
    pos = np.arange(n, dtype=np.uint64)
    for i, (is_pos, shift, bits) in enumerate(shapes):
        if int(same.sum()) <= cap:
            return i
        src = pos if is_pos else m
        d = (src >> np.uint64(shift)) & np.uint64((1 << bits) - 1)
        same &= d == d[t]
    return len(shapes)


def shared_top(n, dtype, j, seed):
    """n keys of `dtype` whose MAPPED keys share their top 8 j bits (j = key bytes: all keys equal) and are random below"""
    a = H.random_bits(n, dtype, seed).copy()
    kb = a.dtype.itemsize
    if j == 0:
        return a
    pattern = 0xA5C3F00F5A3C0FF0 >> (64 - 8 * kb)                           # kb bytes of a fixed pattern; its top j bytes are shared
    m = H.set_top(H.mapped_key(a).view(f"i{kb}"), 8 * kb, 8 * j, pattern >> (8 * (kb - j)))
    return H.unmapped(m.view(f"u{kb}"), dtype)


def shared_top_wide(n, key, bits, seed):
    """the limb form of shared_top: n 16-byte keys ("u128" / "i128", rows of limbs [low, high]) whose MAPPED keys share their
    top `bits` bits (128: all keys equal) and are random below"""
    m = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 2), dtype=np.uint64, endpoint=False)
    pattern = 0xA5C3F00F5A3C0FF0_C33C5AA50FF0F00F                           # its top `bits` bits are shared
    keep = (1 << (128 - bits)) - 1                                          # the bits that stay random
    for limb, shift in ((0, 0), (1, 64)):
        k, p = (keep >> shift) & ((1 << 64) - 1), (pattern >> shift) & ((1 << 64) - 1)
        m[:, limb] = (m[:, limb] & np.uint64(k)) | np.uint64(p & ~k & ((1 << 64) - 1))
    return H.wide_mapped(m, key)


def mapped_ints(a, key, largest=False):
    """the mapped keys of rows of limbs as Python integers (complemented for largest)"""
    flip = (1 << 127 if key == "i128" else 0) ^ ((1 << 128) - 1 if largest else 0)
    return [((int(hi) << 64) | int(lo)) ^ flip for lo, hi in a.tolist()]


def shared_counts_wide(a, k, largest, key):
    """sizes[i], in Python integers: how many 16-byte keys share the digits of the first i 12-bit levels (the last one is 8
    bits wide) with the k-th element of the stable order, i = 0 .. 11"""
    v = mapped_ints(a, key, largest)
    t = v[int(order_of(a, key, largest)[k - 1])]
    sizes, hi = [len(v)], 128
    while hi > 0:
        lo = max(hi - DIGIT_BITS_WIDE, 0)
        v = [x for x in v if x >> lo == t >> lo]                            # (every level above already agrees)
        sizes.append(len(v))
        hi = lo
    return sizes


def direct_depth_wide(a, k, largest, cand_capacity, key, sizes=None):
    """direct_depth for 16-byte keys, keys only: the fewest leading levels whose digits, taken from the k-th element of the
    stable order, are shared by at most cand_capacity elements"""
    cap = min(cand_capacity or DEFAULT_CAND_CAPACITY, max(len(a), 1))
    sizes = sizes or shared_counts_wide(a, k, largest, key)
    return next((i for i, s in enumerate(sizes) if s <= cap), len(sizes) - 1)


WIDE_KEYS = ("u128", "i128")
WIDE_DEPTH_BITS = tuple(sorted({12 * (d - 1) for d in range(1, 12)} | {60, 68, 128}))   # (60 is also 12 * 5)


def wide_depth_cases():
    """(key, bits): the top 12 (d - 1) bits shared reaches depth d = 1 .. 11 at capacity 64 (the level of bits [56, 68)
    straddles the limbs, the last level is 8 bits wide); 60 and 68 bits end inside and behind the straddling level; 120 and
    128 shared bits leave more than 64 equal digits at the last level: the fill"""
    return [(key, bits) for key in WIDE_KEYS for bits in WIDE_DEPTH_BITS]


def wide_depth_input(key, bits):
    return shared_top_wide(DEPTH_LEN, key, bits, 300 + bits)


# a k-th element beyond position 2^20 among equal keys: the top position digit (bits 20 to 31) is not 0
FAR_LEN = (1 << 20) + 4099
FAR_K = (1 << 20) + 2050
FAR_CASES = (("uint32", 4), ("int64", 8))
FAR_CAPACITIES = (64, 1)


def far_input(dtype):
    return np.full(FAR_LEN, H.random_bits(1, dtype, 3)[0], dtype=dtype)


DEPTH_LEN = 20_000
DEPTH_DTYPES = ("uint16", "int32", "float32", "uint64", "float64")


def depth_cases():
    """(dtype, j) for j = 0 .. key bytes"""
    return [(dt, j) for dt in DEPTH_DTYPES for j in range(np.dtype(dt).itemsize + 1)]


def depth_capacities(m):
    return sorted({c for c in (1, 64, m - 1, m, m + 1) if c >= 1})


TIE_LEN = 30_000
TIE_COUNT = 5_000


def tie_case(dtype, seed):
    """TIE_LEN keys: a third below a key T, TIE_COUNT copies of T at scattered positions, the rest above; and a k whose k-th
    key is T with ties on both sides of it.  Returns (keys, k, positions of T)."""
    rng = np.random.default_rng(seed)
    kb = np.dtype(dtype).itemsize
    w = 8 * kb
    m = rng.integers(0, 1 << (w - 2), size=TIE_LEN, dtype=np.uint64)       # mapped keys in the lowest quarter ...
    t = np.uint64(1 << (w - 1))
    above = rng.random(TIE_LEN) < 0.5
    m[above] |= np.uint64(3 << (w - 2))                                     # ... or the highest
    at = np.sort(rng.choice(TIE_LEN, size=TIE_COUNT, replace=False))
    m[at] = t
    keys = H.unmapped(m.astype(f"u{kb}"), dtype)
    below = int((m < t).sum())
    return keys, below + TIE_COUNT // 2, at


def three_values(n, dtype, seed):
    rng = np.random.default_rng(seed)
    vals = H.random_bits(3, dtype, seed + 1)
    return vals[rng.integers(0, 3, size=n)].copy()


def order_sensitive(name, n, dtype):
    """ascending, descending and constant-per-wave runs (in mapped-key order): whole waves on one counter"""
    kb = np.dtype(dtype).itemsize
    w = 8 * kb
    i = np.arange(n, dtype=np.uint64)
    run_bits = (64 * vec(kb)).bit_length() - 1                               # the top digit changes once per load of a wave
    step = np.uint64(1 << (w - digit_bits(kb) - run_bits))
    assert n <= 1 << (digit_bits(kb) + run_bits)
    if name == "ascending":
        m = i * step
    elif name == "descending":
        m = (np.uint64(-(-n >> run_bits) << run_bits) - np.uint64(1) - i) * step   # (from a multiple of the run: runs stay whole)
    else:                                                                   # 64 * vec keys per value: every lane of a wave, every load
        run = np.uint64(64 * vec(kb))
        m = ((i // run) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - w)
    return H.unmapped(m.astype(f"u{kb}"), dtype)


ORDER_FAMILIES = ("ascending", "descending", "constant per wave")


def float_specials(dtype, n, seed):
    """+-0, +-inf, NaNs of both signs with different payloads, among ordinary values"""
    dt = np.dtype(dtype)
    w = 8 * dt.itemsize
    u = f"u{dt.itemsize}"
    exp_all = ((1 << (w - 1)) - 1) ^ ((1 << (23 if w == 32 else 52)) - 1)   # the exponent bits
    sign = 1 << (w - 1)
    special = [0, sign, exp_all, exp_all | sign] + [exp_all | p | s for p in (1, 2, 0x1234, (1 << (22 if w == 32 else 51))) for s in (0, sign)]
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n).astype(dt)
    at = rng.choice(n, size=min(n, 40 * len(special)), replace=False)
    a.view(u)[at] = np.array(special, dtype=u)[np.arange(len(at)) % len(special)]
    return a


def signed_extremes(dtype, n, seed):
    dt = np.dtype(dtype)
    info = np.iinfo(dt)
    rng = np.random.default_rng(seed)
    a = H.random_bits(n, dtype, seed).copy()
    ext = np.array([info.min, info.min + 1, -1, 0, 1, info.max - 1, info.max], dtype=dt)
    at = rng.choice(n, size=min(n, 10 * len(ext)), replace=False)
    a[at] = ext[np.arange(len(at)) % len(ext)]
    return a
