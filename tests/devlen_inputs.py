"""Inputs of the device-length tests (rdst_hip_sort_device_devlen, rdst_hip_sort_pairs_device_devlen): the
lengths m at which the pipeline's kernels change what they do — K3's tile, K1's sweep granularity, K1's first piece border,
the capacity itself — the capacities around the one-workgroup sort's tile, prefixes followed by tails that would show if
they were read, and the numpy statement of the result.  Shared by the CPU test of the inputs
(tests/test_devlen_inputs.py) and the GPU tests, so that both see the same cases."""
import numpy as np

import helpers as H

# Every constant below is the library's own, quoted from rdst_amd/csrc/rdst_kernels.hip (the line it stands on):
HIST_THREADS = 1024              # :241  constexpr int HIST_THREADS = 1024;
CHAINS = 8                       # :155  constexpr int CHAINS = 8;
SMALL_THREADS = 1024             # :2204 constexpr int SMALL_THREADS = SMALL_WAVES * 64;  (SMALL_WAVES = 16)
SMALL_KPT = {1: 16, 2: 16, 4: 16, 8: 8, 16: 4}   # :2205 small_kpt(): key_bytes <= 4 ? 16 : (key_bytes == 8 ? 8 : 4)
PASS_THREADS = 768               # :4335-4338 kPassCfgs: the default shapes all have 12 waves
# keys per thread of the default pass shape (default_cfg :4343, kpt_for :4352): keys up to 4 bytes shape 4 (22), unsigned
# 8-byte keys shape 3 (14), signed and float 8-byte keys shape 5 (10), 16-byte keys shape 2 ((12 / 2) & ~1 = 6)
PASS_KPT = {(1, False): 22, (2, False): 22, (4, False): 22, (1, True): 22, (2, True): 22, (4, True): 22,
            (8, False): 14, (8, True): 10, (16, False): 6, (16, True): 6}
CUS = 256                        # compute units of the one device the library is built for
ERR_LEN_PAST_CAPACITY = 32       # :81   the device error word's bit for a length past the capacity

LENGTH_DTYPES = ("int32", "int64", "uint32", "uint64")
# (key kind, key bytes, value bytes): the four widths of helpers.PAIR_WIDTHS, the kinds u / i / f spread over them
PAIR_CASES = (("u", 4, 4), ("f", 4, 8), ("i", 8, 4), ("f", 8, 8))
# keys only: (dtype name or "u128", key bytes); one signed and one float case among them
KEY_CASES = (("uint8", 1), ("int16", 2), ("uint32", 4), ("float32", 4), ("uint64", 8), ("u128", 16))
KEYS_CAPACITY = 100_003


def hist_gran(key_bytes):
    """keys one unrolled sweep of a K1 block covers (aligned keys): HIST_THREADS lanes x one 16-byte load x 4 (:303 GRAN)"""
    return HIST_THREADS * (16 // key_bytes) * 4


def hist_blocks(n, key_bytes, cus=CUS):
    """K1's grid (:5080 hist_blocks): one block per CU, no more than the data needs, about sqrt(bytes / 4 KiB)"""
    blocks = min(cus, -(-n // hist_gran(key_bytes)))
    balanced = 1
    while balanced * balanced * 4096 < n * key_bytes:
        balanced += 1
    return max(1, min(blocks, balanced))


def hist_piece(n, key_bytes, cus=CUS):
    """keys per K1 block (:248 hist_piece): n over the grid, rounded up to whole sweeps"""
    g, blocks = hist_gran(key_bytes), hist_blocks(n, key_bytes, cus)
    return -(-(-(-n // blocks)) // g) * g


def pass_tile(key_bytes, mapped):
    """keys per tile of the keys-only passes at these lengths"""
    return PASS_THREADS * PASS_KPT[(key_bytes, mapped)]


def small_tile(key_bytes):
    """the longest slice the one-workgroup sort takes (run_pipeline picks it from a length the host knows)"""
    return SMALL_THREADS * SMALL_KPT[key_bytes]


def border_lengths(capacity, tile, key_bytes):
    """the lengths m of one capacity, each with the border it stands for; sorted, without repeats, all <= capacity"""
    g, piece = hist_gran(key_bytes), hist_piece(capacity, key_bytes)
    named = {0: "empty", 1: "one", 2: "two", 3: "three",
             tile - 1: "tile - 1", tile: "tile", tile + 1: "tile + 1",
             g - 1: "sweep - 1", g: "sweep", g + 1: "sweep + 1",
             piece - 1: "piece - 1", piece: "piece", piece + 1: "piece + 1",
             capacity - 1: "capacity - 1", capacity: "capacity",
             (capacity // 2) | 1: "odd middle"}
    return sorted((m, what) for m, what in named.items() if 0 <= m <= capacity)


def pair_capacity(key_bytes, val_bytes):
    """37 tiles and a half: several tiles on each of the 8 chains"""
    return H.pair_lengths(key_bytes, val_bytes)[1]


def pair_lengths(key_bytes, val_bytes):
    return border_lengths(pair_capacity(key_bytes, val_bytes), H.pair_tile(key_bytes, val_bytes), key_bytes)


def key_capacities(key_bytes):
    """2, 3, and both sides of the one-workgroup sort's tile"""
    t = small_tile(key_bytes)
    return 2, 3, t - 1, t, t + 1


def key_lengths(key, key_bytes):
    mapped = key != "u128" and np.dtype(key).kind != "u"
    return border_lengths(KEYS_CAPACITY, pass_tile(key_bytes, mapped), key_bytes)


def small_lengths(capacity):
    """the lengths tried at a capacity around the one-workgroup tile"""
    return sorted({0, 1, 2, capacity // 2 + 1, capacity - 1, capacity} & set(range(capacity + 1)))


def random_keys(n, key, seed):
    """random bit patterns: a numpy array of dtype `key`, or (n, 2) uint64 limbs [low, high] for "u128" """
    if key == "u128":
        return np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 2), dtype=np.uint64, endpoint=False)
    return H.random_bits(n, key, seed).copy()


def order_of(keys):
    """the stable order of the keys (rows of limbs for "u128": high limb first)"""
    if keys.ndim == 2:
        return np.lexsort((keys[:, 0], keys[:, 1]))
    return np.argsort(H.mapped_key(keys), kind="stable")


def expected_prefix_sorted(keys, m, vals=None):
    """THE result of a device-length sort: the first m keys in stable mapped-key order, the tail as it was"""
    order = np.concatenate([order_of(keys[:m]), np.arange(m, len(keys))]).astype(np.int64)
    return keys[order] if vals is None else (keys[order], vals[order])


def whole_array_order(keys, m):
    """the same permutation stated as ONE stable sort of the whole array: the key of element i is its mapped key for i < m
    and "above everything, in position order" for the tail — (0, mapped key) for the prefix, (1, i) for the tail"""
    n = len(keys)
    mk = H.mapped_key(keys).astype(np.uint64)
    tail = np.arange(n) >= m
    second = np.where(tail, np.arange(n, dtype=np.uint64), mk)
    return np.lexsort((second, tail.astype(np.uint8)))


# ---- tails that would show if they were read ---------------------------------------------------------------------------
TAIL_FAMILIES = ("tail below", "tail varies", "sorted prefix", "one swap")


def tail_case(name, capacity, m, dtype, seed=0):
    """`capacity` keys of `dtype`, a prefix of m and a tail of capacity - m keys:
      "tail below"     every tail key is below every prefix key (a tail that is read is sorted in front)
      "tail varies"    the prefix is constant in two of its bytes — those levels are skipped — and the tail varies in them
      "sorted prefix"  the prefix is sorted already and the tail is not: nothing may change
      "one swap"       prefix + tail are one sorted run apart from one swap inside the prefix (an inversion test that
                       looked at the whole array, or only at the tail, would decide differently from one on the prefix)"""
    dt = np.dtype(dtype)
    w = 8 * dt.itemsize
    ut = np.dtype(f"u{dt.itemsize}")
    rng = np.random.default_rng([seed, capacity, m, TAIL_FAMILIES.index(name), dt.itemsize])

    def rand(n, lo, hi):                                    # mapped keys in [lo, hi]
        return rng.integers(lo, hi, size=n, dtype=np.uint64, endpoint=True).astype(ut)

    half, top = 1 << (w - 1), (1 << w) - 1
    if name == "tail below":
        mk = np.concatenate([rand(m, half, top), rand(capacity - m, 0, half - 1)])
    elif name == "tail varies":
        mk = rand(capacity, 0, top)
        const = ut.type(0xFF << 8 | 0xFF << (w - 16))       # bytes 1 and w / 8 - 2
        mk[:m] = (mk[:m] & ~const) | ut.type(0x5A << 8 | 0xA5 << (w - 16))
    elif name == "sorted prefix":
        mk = np.concatenate([np.sort(rand(m, 0, top)), rand(capacity - m, 0, half - 1)])
    else:
        assert name == "one swap", name
        step = top // capacity                              # strictly increasing: i * step + a random part below step
        mk = np.arange(capacity, dtype=ut) * ut.type(step) + rand(capacity, 0, step - 1)
        i = m // 3
        mk[[i, i + 1]] = mk[[i + 1, i]]
    keys = H.unmapped(mk, dt.name)
    assert H.same_bits(H.mapped_key(keys), mk)
    return keys


# the same for the widths tail_case's two constant bytes do not fit: (key, the levels at which the "tail varies" prefix is
# constant) — one pass is left for int16 and thirteen for u128, an odd number, so copyback_devlen_kernel moves exactly m keys
NARROW_WIDE_TAILS = (("int16", (1,)), ("u128", (0, 1, 2)))
NARROW_WIDE_FAMILIES = ("tail varies", "sorted prefix")


def tail_case_levels(name, capacity, m, key, levels, seed=0):
    """tail_case for "int16" and "u128" (rows of limbs [low, high]):
      "tail varies"    the prefix is constant at `levels` of the mapped key — K2 skips them if it looks at the prefix alone —
                       and the tail varies in them
      "sorted prefix"  the prefix is sorted already and the tail is not, and lies below the prefix's largest key"""
    if name == "tail varies":
        if key == "u128":
            keys = H.wide_with_constant_levels(capacity, key, (), seed=[seed, capacity, m])
            keys[:m] = H.wide_with_constant_levels(m, key, levels, seed=[seed, m])
            return keys
        keys = H.random_bits(capacity, key, seed + capacity).copy()
        keys[:m] = H.keys_with_constant_levels(m, key, levels, seed + m)
        return keys
    assert name == "sorted prefix", name
    if key == "u128":
        keys = random_keys(capacity, key, seed + capacity)
        keys[m:, 1] >>= np.uint64(1)                            # the tail: in the lower half
        keys[:m] = keys[:m][order_of(keys[:m])]
        return keys
    return tail_case(name, capacity, m, key, seed)
