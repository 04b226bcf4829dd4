"""Inputs and numpy statements for the order statistics (rdst_hip_select_device): THE result as a stable
argsort over the mapped key, the round loop of the multi-rank radix select restated (groups, below, m, depth, candidates,
exhaustion), so that a test can say what a case reaches and compare it with what the device reports
(rdst_hip_debug_select_state), and the case lists of tests/test_gpu_select.py.

Keys are 1-D numpy arrays of a built-in dtype, or (n, 2) uint64 rows of limbs [low, high] with key="u128" / "i128"."""
import numpy as np

import helpers as H
import topk_inputs as T

# the library's constants (tests/test_select_inputs.py compares them with rdst_hip_select_limits)
MAX_RANKS = 64
DIGIT0_BITS_WIDE = 12
DIGIT0_BITS_BYTE = 8
DIGIT_BITS = 8
POSITION_BITS = 32
DEFAULT_CAND_CAPACITY = 1 << 24
DEPTH_LEN = T.DEPTH_LEN


def digit0_bits(kb):
    return DIGIT0_BITS_BYTE if kb == 1 else DIGIT0_BITS_WIDE


def level_shapes(kb, indexed):
    """(is a position level, shift, bits) of every level a round can take, most significant first: the first digit, the rest
    of the key in 8-bit digits (the last one is the narrow one), then the position's four bytes"""
    d0 = digit0_bits(kb)
    out = [(False, 8 * kb - d0, d0)]
    for pos, bits in ((False, 8 * kb - d0), (True, POSITION_BITS))[:2 if indexed else 1]:
        hi = bits
        while hi > 0:
            lo = max(hi - DIGIT_BITS, 0)
            out.append((pos, lo, hi - lo))
            hi = lo
    return out


def max_levels(kb, indexed):
    return len(level_shapes(kb, indexed))


def key_levels(kb):
    return max_levels(kb, False)


def name_of(a, key=None):
    return key if key else a.dtype.name


def expected_select(a, ranks, largest=False, key=None):
    """THE result: (keys, positions) of the elements at `ranks` of a stable argsort by the mapped key (complemented for
    largest), slot i for ranks[i]"""
    order = T.order_of(a, key, largest)
    at = order[np.asarray(ranks, dtype=np.int64)]
    return a[at], at.astype(np.int64)


def restate_round(a, ranks, largest=False, indexed=False, cand_capacity=0, key=None):
    """One round (at most MAX_RANKS ranks, ascending) as the device runs it.  Returns the state rdst_hip_debug_select_state
    reports — levels, groups, candidates, exhausted —, `trace` (the number of groups after every level), `m` (the sum of the
    groups' sizes at the end) and `positions`: per rank the input position of its answer (keys only and exhausted: of one
    element that holds the answer's key)."""
    assert 1 <= len(ranks) <= MAX_RANKS and list(ranks) == sorted(ranks)
    name = name_of(a, key)
    kb = T.key_bytes(name)
    n = len(a)
    cap = min(cand_capacity or DEFAULT_CAND_CAPACITY, max(n, 1))
    hi, lo = T.mapped_limbs(a, name, largest)
    pos = np.arange(n, dtype=np.uint64)
    zeros = np.zeros(n, dtype=np.uint64)
    order = T.order_of(a, key, largest)
    groups = [{"on": np.ones(n, dtype=bool), "below": 0, "m": n}]            # ascending prefix order
    grp = [0] * len(ranks)
    levels, exhausted, trace = 0, 0, []
    shapes = level_shapes(kb, indexed)
    if n > cap:
        for i, (is_pos, shift, bits) in enumerate(shapes):
            d = T._digit(zeros, pos, 8, shift, bits) if is_pos else T._digit(hi, lo, kb, shift, bits)
            new_groups, new_grp, seen = [], [], {}
            for r, g in zip(ranks, grp):
                G = groups[g]
                counts = np.bincount(d[G["on"]], minlength=1 << bits)
                cum = np.cumsum(counts)
                b = int(np.searchsorted(cum, r - G["below"], side="right"))  # cum[b - 1] <= r - below < cum[b]
                if (g, b) not in seen:                                       # ranks ascend: so do (group, digit)
                    seen[(g, b)] = len(new_groups)
                    new_groups.append({"on": G["on"] & (d == b), "below": G["below"] + int(cum[b] - counts[b]), "m": int(counts[b])})
                new_grp.append(seen[(g, b)])
            groups, grp = new_groups, new_grp
            levels = i + 1
            trace.append(len(groups))
            total = sum(G["m"] for G in groups)
            last = i + 1 == len(shapes)
            if last:
                exhausted = 1
            if last or total <= cap:
                break
    total = sum(G["m"] for G in groups)
    positions = []
    for r, g in zip(ranks, grp):
        G = groups[g]
        members = order[G["on"][order]]                                      # the group's elements in the stable order
        assert len(members) == G["m"] and 0 <= r - G["below"] < G["m"]
        positions.append(int(members[0] if exhausted else members[r - G["below"]]))
    return {"levels": levels, "groups": len(groups), "candidates": 0 if exhausted else total, "exhausted": exhausted, "trace": trace, "m": total,
            "positions": positions}


def rounds_of(ranks):
    """the rounds of a call: lists of (rank, slot), ascending by rank, equal ranks in slot order, MAX_RANKS at a time"""
    pairs = sorted(((int(r), i) for i, r in enumerate(ranks)), key=lambda p: p[0])
    return [pairs[i:i + MAX_RANKS] for i in range(0, len(pairs), MAX_RANKS)]


def restate(a, ranks, largest=False, indexed=False, cand_capacity=0, key=None):
    """The whole call: (positions in the caller's slot order, the state of every round)"""
    out = [0] * len(ranks)
    states = []
    for rnd in rounds_of(ranks):
        st = restate_round(a, [r for r, _ in rnd], largest, indexed, cand_capacity, key)
        for (_r, slot), p in zip(rnd, st["positions"]):
            out[slot] = p
        states.append(st)
    return np.array(out, dtype=np.int64), states


def state_fields(st):
    return {f: st[f] for f in ("levels", "groups", "candidates", "exhausted")}


# ---- the case lists ------------------------------------------------------------------------------------------------------------

def rank_sets(n):
    """the rank sets of the border cases"""
    sets = [[0], [n - 1], [0, n - 1, n // 2], [n // 2, n // 2, 0, n // 2], sorted({n - 1, n // 2, n // 3, 0}, reverse=True)]
    return [s for i, s in enumerate(sets) if s not in sets[:i]]


def spaced_ranks(n, count):
    """`count` evenly spaced ranks inside 0 .. n - 1"""
    return [int((2 * i + 1) * n // (2 * count)) for i in range(count)]


def parting_input(dtype, level, seed):
    """DEPTH_LEN keys whose MAPPED keys agree above the digit of `level` (0-based, a key level of this dtype), hold one of two
    digit values there, half and half, and are random below: two ranks, one in each half, share every earlier level and part
    at `level`.  Returns (keys, the two ranks)."""
    kb = np.dtype(dtype).itemsize
    _pos, shift, bits = level_shapes(kb, False)[level]
    rng = np.random.default_rng(seed)
    w = 8 * kb
    full = (1 << w) - 1
    pattern = (0xA5C3F00F5A3C0FF0 >> (64 - w)) & full
    low_mask = (1 << shift) - 1
    top = pattern & full & ~((1 << (shift + bits)) - 1)
    m = rng.integers(0, 1 << 63, size=DEPTH_LEN, dtype=np.uint64) & np.uint64(low_mask)
    half = rng.random(DEPTH_LEN) < 0.5
    da, db = 1, (1 << bits) - 2
    m |= np.uint64(top) | np.where(half, np.uint64(db << shift), np.uint64(da << shift))
    keys = H.unmapped(m.astype(f"u{kb}"), dtype)
    n_a = int((~half).sum())
    return keys, [n_a // 2, n_a + (DEPTH_LEN - n_a) // 2]


def one_bucket_input(dtype, seed):
    """DEPTH_LEN keys whose mapped keys share the first digit and are random below"""
    kb = np.dtype(dtype).itemsize
    return T.shared_top(DEPTH_LEN, dtype, 0, seed) if kb == 1 else _shared_first_digit(dtype, seed)


def _shared_first_digit(dtype, seed):
    kb = np.dtype(dtype).itemsize
    w = 8 * kb
    d0 = digit0_bits(kb)
    m = np.random.default_rng(seed).integers(0, 1 << 63, size=DEPTH_LEN, dtype=np.uint64) & np.uint64((1 << (w - d0)) - 1)
    m |= np.uint64(0x9A7 << (w - d0))
    return H.unmapped(m.astype(f"u{kb}"), dtype)


HEAVY_COUNT = 5000


def heavy_input(dtype, seed):
    """DEPTH_LEN random keys, HEAVY_COUNT of them one value at scattered positions.  Returns (keys, ranks): ranks inside the
    heavy run (both ends and the middle) and light ones on both sides."""
    rng = np.random.default_rng(seed)
    a = H.random_bits(DEPTH_LEN, dtype, seed).copy()
    at = np.sort(rng.choice(DEPTH_LEN, size=HEAVY_COUNT, replace=False))
    v = a[at[0]]
    a[at] = v
    m = H.mapped_key(a)
    below = int((m < H.mapped_key(a[at[:1]])[0]).sum())
    ranks = sorted({0, below // 2, max(below - 1, 0), below, below + HEAVY_COUNT // 2, below + HEAVY_COUNT - 1,
                    min(below + HEAVY_COUNT, DEPTH_LEN - 1), DEPTH_LEN - 1})
    return a, ranks


def capacities(m):
    """small capacities, and both sides of the sum of the groups' sizes `m`"""
    return sorted({c for c in (1, 2, 64, m - 1, m) if c >= 1})


WIDE_BITS = (0, 60, 68, 128)
