"""Inputs of the run-length tests (rdst_hip_runs_device): the lengths and head positions at which the
kernel changes what it does — its tile, a tile without a head, a look-back longer than its window —, keys that differ in one
half only, the float keys whose BITS decide, and the numpy statement of the result.  Shared by the CPU test of the inputs
(tests/test_runs_inputs.py) and the GPU tests, so that both see the same cases."""
import numpy as np

# The library's own, quoted from rdst_amd/csrc/rdst_runs_layout.h (tests/test_runs_inputs.py looks the lines up):
THREADS = 256                # constexpr uint32_t THREADS = 256;
ROWS = {1: 4, 2: 8, 4: 8, 8: 16, 16: 16}   # constexpr uint32_t rows(uint32_t elem_bytes) { return elem_bytes >= 8 ? 16 : (elem_bytes == 1 ? 4 : 8); }
LOOKBACK_WINDOW = 8          # constexpr uint32_t LOOKBACK_WINDOW = 8;
ERR_LEN_PAST_CAPACITY = 32   # the device error word's bit for a length past `len`
ERR_RUNS_TRUNCATED = 64      # ... and for more runs than the capacity

# every width and kind: (key name, bytes); "u128" / "i128": rows of 8-byte limbs [low, high]
KEY_CASES = (("uint8", 1), ("int8", 1), ("uint16", 2), ("int16", 2), ("uint32", 4), ("int32", 4), ("float32", 4), ("uint64", 8), ("int64", 8),
             ("float64", 8), ("u128", 16), ("i128", 16))
_ODD = 0x9E3779B97F4A7C15    # an odd multiplier: r -> r * _ODD is one-to-one modulo every power of two


def tile(key_bytes):
    """T: keys per tile"""
    return THREADS * ROWS[key_bytes] * 16 // key_bytes


def wide(key):
    return key in ("u128", "i128")


def bits(keys):
    """the keys as unsigned integers of their width (128-bit keys: the (n, 2) limbs as they are)"""
    return keys if keys.ndim == 2 else keys.view(f"u{keys.dtype.itemsize}")


def heads_of(keys):
    """THE definition: position 0, and every position whose bits differ from the ones in front of it"""
    b = bits(keys)
    if len(b) == 0:
        return np.zeros(0, dtype=bool)
    differs = b[1:] != b[:-1]
    if b.ndim == 2:
        differs = differs.any(axis=1)
    return np.r_[True, differs]


def expected(keys, m=None):
    """(run keys, starts, R) of the first m keys: keys[heads], flatnonzero(heads), heads.sum()"""
    keys = keys if m is None else keys[:m]
    h = heads_of(keys)
    return keys[h], np.flatnonzero(h), int(h.sum())


def expected_by_loop(keys):
    """the same by a plain loop over Python ints"""
    b = bits(keys)
    rows = [tuple(int(x) for x in r) for r in b] if b.ndim == 2 else [int(x) for x in b]
    starts = [i for i in range(len(rows)) if i == 0 or rows[i] != rows[i - 1]]
    return starts, len(starts)


def keys_from_heads(heads, key, half=None, seed=0):
    """keys of type `key` whose heads are exactly `heads` (a bool array, heads[0] True): run r holds (r + seed) * _ODD cut to the
    key's width, so neighbouring runs differ.  128-bit keys, and 8-byte ones with `half`: "high" / "low" keeps the other half
    of every key constant, so that the runs differ in that half only."""
    heads = np.asarray(heads, dtype=bool)
    run = (np.cumsum(heads, dtype=np.uint64) - np.uint64(1) + np.uint64(seed)) if len(heads) else np.zeros(0, dtype=np.uint64)
    val = run * np.uint64(_ODD)
    if wide(key):
        out = np.empty((len(heads), 2), dtype=np.uint64)
        out[:, 0] = np.uint64(0x0123456789ABCDEF) if half == "high" else val
        out[:, 1] = np.uint64(0xFEDCBA9876543210) if half == "low" else (val if half == "high" else run)
        return out
    dt = np.dtype(key)
    if half is not None:
        assert dt.itemsize == 8, "halves: 8- and 16-byte keys"
        r32 = (run * np.uint64(_ODD >> 32 | 1)) & np.uint64(0xFFFFFFFF)
        val = (r32 << np.uint64(32)) | np.uint64(0x89ABCDEF) if half == "high" else (np.uint64(0x76543210) << np.uint64(32)) | r32
    return val.astype(f"u{dt.itemsize}").view(dt)


def heads_at(n, positions):
    h = np.zeros(n, dtype=bool)
    if n:
        p = np.asarray(positions, dtype=np.int64)
        h[p[(p >= 0) & (p < n)]] = True
        h[0] = True
    return h


def random_runs(n, rng, longest=9):
    """heads of runs of random length 1 .. longest"""
    lengths = rng.integers(1, longest, size=n + 1, endpoint=True)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    return heads_at(n, starts[starts < n])


def border_lengths(t):
    return (0, 1, 2, t - 1, t, t + 1, 2 * t, 3 * t + 5)


def shapes(key_bytes):
    """name -> heads, for one key width: what a tile border, a tile without a head and a long walk look like"""
    t = tile(key_bytes)
    rng = np.random.default_rng([7, key_bytes])
    out = {}
    for n in border_lengths(t):
        out[f"random runs, {n} keys"] = random_runs(n, rng)
    n = 3 * t + 5
    for p in (t - 1, t, t + 1):
        out[f"heads at 0 and {p}"] = heads_at(n, [p])
    out["heads at T - 1, T and T + 1"] = heads_at(n, [t - 1, t, t + 1])
    out["all equal"] = heads_at(n, [])
    out["all distinct"] = np.ones(n, dtype=bool)
    # six tiles; one run covers tiles 1 .. 3 whole (it starts inside tile 0 and ends inside tile 4): three tiles without a head
    six = random_runs(6 * t, rng)
    six[t - 3:4 * t + 2] = False
    six[t - 3] = True
    out["one run over tiles 1 .. 3"] = six
    # 40 tiles of one key, then a tile of distinct ones: the last tile's walk is longer than the look-back window
    assert 40 > LOOKBACK_WINDOW
    far = heads_at(41 * t, [])
    far[40 * t:] = True
    out["40 equal tiles, then a distinct one"] = far
    return out


def float_cases():
    """name -> (keys, starts): float keys whose bits decide, not their values"""
    out = {}
    for dt, ut, qnan, payload in ((np.float32, np.uint32, 0x7FC00000, 0x7FC00001), (np.float64, np.uint64, 0x7FF8000000000000, 0x7FF8000000000001)):
        def f(*words, ut=ut, dt=dt):
            return np.array(words, dtype=ut).view(dt)
        sign = 1 << (8 * np.dtype(ut).itemsize - 1)
        name = np.dtype(dt).name
        out[f"{name}: -0.0 and +0.0 are different keys"] = (f(0, 0, sign, sign, 0), [0, 2, 4])
        out[f"{name}: two NaN payloads are different keys"] = (f(qnan, payload, payload, qnan | sign), [0, 1, 3])
        out[f"{name}: equal NaN bits are one key"] = (f(qnan, qnan, qnan, payload, payload), [0, 3])
    return out


def half_cases():
    """(name, key, half): 16- and 8-byte keys whose runs differ in the high half only, or in the low half only"""
    return [(f"{key}, runs differ in the {half} half only", key, half) for key in ("u128", "i128", "uint64", "int64", "float64") for half in ("high", "low")]
