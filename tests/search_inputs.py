"""Inputs of the binary-search tests (rdst_hip_search_device): the lengths and needle counts at which the
kernel changes what it does — its tile of needles, its splitter table, the window it stages in LDS —, haystacks and needles
built in the MAPPED order (present keys, keys between two neighbours, keys below the first and above the last, the type's
extremes), the float keys whose BITS decide, and the numpy statement of the result.  Shared by the CPU test of the inputs
(tests/test_search_inputs.py) and the GPU tests, so that both see the same cases.

Keys are 1-D numpy arrays of a built-in dtype, or (n, 2) uint64 rows of limbs [low, high] with key "u128" / "i128"."""
import numpy as np

import helpers as H
from runs_inputs import KEY_CASES, wide  # noqa: F401  (every width and kind; the GPU tests take them from here)

# The library's own, quoted from rdst_amd/csrc/rdst_search_layout.h (tests/test_search_inputs.py looks the lines up):
THREADS = 256                                        # constexpr uint32_t THREADS = 256;
NEEDLES_PER_THREAD = {1: 16, 2: 8, 4: 8, 8: 8, 16: 4}   # ... needles_per_thread(uint32_t elem_bytes) { return elem_bytes == 1 ? 16 : (elem_bytes == 16 ? 4 : 8); }
SPLITTERS = 1024                                     # constexpr uint32_t SPLITTERS = 1024;
WINDOW = {1: 8192, 2: 8192, 4: 8192, 8: 4096, 16: 2048}  # ... window(uint32_t elem_bytes) { return elem_bytes == 16 ? 2048 : (elem_bytes == 8 ? 4096 : 8192); }
ERR_LEN_PAST_CAPACITY = 32                           # the device error word's bit for a length past `len`


def tile(key_bytes):
    """T: needles per workgroup tile"""
    return THREADS * NEEDLES_PER_THREAD[key_bytes]


def key_bytes(key):
    return 16 if wide(key) else np.dtype(key).itemsize


def haystack_lengths(kb):
    s, w = SPLITTERS, WINDOW[kb]
    return (0, 1, 2, s - 1, s, s + 1, w - 1, w, w + 1, 3 * w + 5)


def needle_counts(kb):
    t = tile(kb)
    return (1, t - 1, t, t + 1, 3 * t + 5)


def mapped(keys, key):
    """the keys' images in the sort's order: numpy unsigned integers (helpers.mapped_key), for 16-byte keys an object array
    of Python integers"""
    if not wide(key):
        return H.mapped_key(keys)
    m = H.wide_mapped(keys, key)
    out = np.empty(len(m), dtype=object)
    out[:] = [(int(hi) << 64) | int(lo) for lo, hi in m.tolist()]
    return out


def expected(sorted_keys, needles, key, m=None):
    """THE definition: (lower, upper) = np.searchsorted(mapped haystack[:m], mapped needles, "left" / "right")"""
    hay = mapped(sorted_keys if m is None else sorted_keys[:m], key)
    q = mapped(needles, key)
    return np.searchsorted(hay, q, side="left").astype(np.int64), np.searchsorted(hay, q, side="right").astype(np.int64)


def expected_by_loop(sorted_keys, needles, key, m=None):
    """the same by a plain count over Python ints: keys strictly before the needle, keys before or equal"""
    hay = [int(x) for x in mapped(sorted_keys if m is None else sorted_keys[:m], key)]
    q = [int(x) for x in mapped(needles, key)]
    return [sum(h < x for h in hay) for x in q], [sum(h <= x for h in hay) for x in q]


def from_mapped(m, key):
    """the keys whose mapped images are the Python / numpy integers `m`"""
    if not wide(key):
        return H.unmapped(np.asarray(m, dtype=f"u{np.dtype(key).itemsize}"), key)
    limbs = np.array([[int(x) & (2**64 - 1), int(x) >> 64] for x in m], dtype=np.uint64).reshape(len(m), 2)
    return H.wide_mapped(limbs, key)


def _random_mapped(rng, n, bits, lo, hi):
    """n Python-int-safe random integers in [lo, hi) as an object array (any width up to 128 bits)"""
    span = hi - lo
    parts = rng.integers(0, 1 << 62, size=(n, 3), dtype=np.uint64)
    out = np.empty(n, dtype=object)
    out[:] = [lo + ((int(a) << 124 | int(b) << 62 | int(c)) % span) for a, b, c in parts.tolist()]
    return out


def haystack(key, m, seed, distinct=None):
    """m sorted keys of `key`: mapped images in the MIDDLE HALF of the range, low bit clear (image | 1 is then a key between
    two neighbours that is not present), drawn from `distinct` values (default: about m / 3, so that keys repeat)"""
    bits = 8 * key_bytes(key)
    rng = np.random.default_rng([seed, m, bits])
    pool = _random_mapped(rng, max(1, m // 3 if distinct is None else distinct), bits, 1 << (bits - 2), 3 << (bits - 2))
    pool = np.array([int(x) & ~1 for x in pool], dtype=object)
    picks = np.sort(pool[rng.integers(0, len(pool), size=m)]) if m else np.empty(0, dtype=object)
    return from_mapped(list(picks), key)


def needles_for(hay, key, n, seed):
    """n needles for the sorted haystack `hay`: present keys, keys between two neighbours (a present image | 1), keys below the
    first and above the last, and the type's extremes (mapped 0 and all ones, and the bit patterns 0 and sign-bit-only), shuffled"""
    bits = 8 * key_bytes(key)
    rng = np.random.default_rng([seed, n, bits, len(hay)])
    top = (1 << bits) - 1
    special = [0, top, 1 << (bits - 1), (1 << (bits - 1)) - 1, 1, top - 1]              # the extremes of every kind's map
    special += [int(x) for x in _random_mapped(rng, 4, bits, 0, 1 << (bits - 2))]       # below every key of the haystack
    special += [int(x) for x in _random_mapped(rng, 4, bits, 3 << (bits - 2), top)]     # above every one
    if len(hay):
        hm = mapped(hay, key)
        present = [int(x) for x in hm[rng.integers(0, len(hay), size=n)]]
        special += [int(hm[0]), int(hm[-1]), int(hm[0]) - 1, int(hm[-1]) + 1]
    else:
        present = [int(x) for x in _random_mapped(rng, n, bits, 0, top)]
    out = [x | 1 if i % 3 == 2 else x for i, x in enumerate(present)]                     # a third of them between two neighbours
    spots = rng.permutation(n)[:len(special)]
    for s, x in zip(spots.tolist(), special):                                             # (n == 1: one special needle)
        out[s] = x
    return from_mapped(out, key)


def float_cases():
    """name -> (sorted haystack, needles, lower, upper): float keys whose bits decide, not their values.  The haystack holds
    -NaN, -inf, -1, -0.0, +0.0, 1, +inf, +NaN and two NaN payloads, with 1 twice; the needles are every one of them, a NaN
    that is not there and 0.5"""
    out = {}
    for dt, ut, exp_mask, quiet in ((np.float32, np.uint32, 0x7F800000, 0x00400000), (np.float64, np.uint64, 0x7FF0000000000000, 0x0008000000000000)):
        sign = 1 << (8 * np.dtype(ut).itemsize - 1)
        one = int(np.array([1.0], dtype=dt).view(ut)[0])
        half = int(np.array([0.5], dtype=dt).view(ut)[0])
        qnan, payload = exp_mask | quiet, exp_mask | quiet | 1
        #      -NaN(payload)   -NaN         -inf             -1          -0.0  +0.0  1    1    +inf      +NaN  +NaN(payload)
        hay = [sign | payload, sign | qnan, sign | exp_mask, sign | one, sign, 0, one, one, exp_mask, qnan, payload]
        needles = hay + [exp_mask | quiet | 2, half, sign | half]
        lower = [0, 1, 2, 3, 4, 5, 6, 6, 8, 9, 10, 11, 6, 4]
        upper = [1, 2, 3, 4, 5, 6, 8, 8, 9, 10, 11, 11, 6, 4]
        out[np.dtype(dt).name] = (np.array(hay, dtype=ut).view(dt), np.array(needles, dtype=ut).view(dt), lower, upper)
    return out


def ramp(key, m, plateau=None):
    """m sorted DISTINCT keys (images: a base in the second quarter of the range, then steps of 2; not for 1-byte keys);
    plateau=(start, length): that stretch repeats the key at `start` instead — a run of equal keys"""
    bits = 8 * key_bytes(key)
    assert bits >= 16 and 2 * m < (1 << (bits - 2))
    img = [(1 << (bits - 2)) + 2 * i for i in range(m)]
    if plateau is not None:
        start, length = plateau
        img[start:start + length] = [img[start]] * length
    return from_mapped(img, key)


def take(keys, index):
    return keys[np.asarray(index)]


def interleaved(n, tiles):
    """the permutation that deals n = tiles * T sorted needles out to the tiles like cards: tile r gets the needles
    r, r + tiles, r + 2 tiles, ..., so every tile spans all but `tiles - 1` of the sorted needles"""
    assert n % tiles == 0
    return np.arange(n).reshape(n // tiles, tiles).T.reshape(-1)
