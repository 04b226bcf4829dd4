"""Inputs and numpy statements for the segmented partial sort (rdst_hip_topk_segments_device): the case lists
of tests/test_gpu_topk_segments.py, THE result — topk_inputs.expected_topk per segment with k_s = min(k, n_s) —, the plan
(the class of a segment of n_s keys at a given k, and the work list in the entry's order) and the stream class's select
restated: levels until c_below + m <= TILE.

Keys are 1-D numpy arrays of a built-in dtype, or (n, 2) uint64 rows of limbs with key="u128" / "i128"; offsets count keys."""
import numpy as np

import helpers as H
import topk_inputs as T

# the library's shapes, quoted from rdst_amd/csrc/rdst_segments_layout.h (tests/test_topk_segments_abi.py compares them with
# rdst_hip_topk_segments_limits)
BLOCK_THREADS = 1024
STREAM_MAX_DEFAULT = 1 << 17
CLASSES = ("wave", "block", "stream", "far")


def wave_max(kb):
    return 64 * (4 if kb == 16 else 8)


def block_max(kb, indexed):
    vb = 4 if indexed else 0                                                # the position travels as a u32 beside the key
    kpt = 8 if vb and kb + vb > 8 else (16 if kb <= 4 else (8 if kb == 8 else 4))
    return BLOCK_THREADS * kpt


def limits(kb, indexed, stream_max=0):
    bm = block_max(kb, indexed)
    return wave_max(kb), bm, max(bm, stream_max or STREAM_MAX_DEFAULT), bm


def class_of(n, k, kb, indexed, stream_max=0):
    """0 .. 3 = wave, block, stream, far for a segment of n >= 1 keys"""
    wm, bm, sm, ksm = limits(kb, indexed, stream_max)
    if n <= wm:
        return 0
    if n <= bm:
        return 1
    return 2 if n <= sm and k <= ksm else 3


def plan(offsets, k, kb, indexed, stream_max=0):
    """(items, counts, longest_far) as rdst_topk_segments_plan gives them: wave class in segment order; block class and then
    stream class, each longest first with ties in segment order; far class in segment order"""
    off = [int(o) for o in offsets]
    per = [[], [], [], []]
    for s in range(len(off) - 1):
        n = off[s + 1] - off[s]
        if n and k:
            per[class_of(n, k, kb, indexed, stream_max)].append((off[s], n, s))
    for c in (1, 2):
        per[c].sort(key=lambda it: -it[1])                                  # (stable: ties stay in segment order)
    return per[0] + per[1] + per[2] + per[3], tuple(len(p) for p in per), max((it[1] for it in per[3]), default=0)


def expected(a, offsets, k, largest=False, key=None):
    """per segment: (keys, positions) of its first k_s elements in the stable order — the positions local to the segment"""
    return [T.expected_topk(a[int(lo):int(hi)], min(k, int(hi) - int(lo)), largest, key) for lo, hi in zip(offsets[:-1], offsets[1:])]


def stream_depth(seg, k, largest, tile, key=None):
    """The stream class's select on one segment (longer than `tile`, k <= tile): a digit per level, most significant first,
    over the keys still on the prefix, until c_below + m <= tile or the digits are exhausted.  Returns (levels, c_below, m)."""
    name = key if key else seg.dtype.name
    kb = T.key_bytes(name)
    hi, lo = T.mapped_limbs(seg, name, largest)
    if not T.is_wide(name) and kb < 8 and largest:
        lo = lo & np.uint64((1 << (8 * kb)) - 1)                            # the complement inside the key's width
    on = np.ones(len(seg), dtype=bool)
    levels, c_below, m = 0, 0, len(seg)
    for _pos, shift, bits in T.level_shapes(kb, False):
        if c_below + m <= tile:
            break
        d = T._digit(hi, lo, kb, shift, bits)
        counts = np.bincount(d[on], minlength=1 << bits)
        cum = np.cumsum(counts)
        b = int(np.searchsorted(cum, k - c_below, side="left"))
        c_below += int(cum[b] - counts[b])
        m = int(counts[b])
        on &= d == b
        levels += 1
    return levels, c_below, m


# ---- case lists ------------------------------------------------------------------------------------------------------------

def segment_lengths(wm, bm):
    return [0, 1, 2, 63, 64, 65, wm - 1, wm, wm + 1, 1023, 1024, 1025, bm - 1, bm, bm + 1, bm + 1025, 2 * bm + 3, 4 * bm + 7]


def table_ks(wm, bm):
    """the k of the table of segment_lengths: beside 1, 2, 63, 64 and 65 the lengths wm, 1024 and bm, which are n_s - 1, n_s
    and n_s + 1 of their neighbours in the table (as 1, 2, 64 are for the short rows); bm + 1 sends the segments beyond bm to
    the far class"""
    return sorted({1, 2, 63, 64, 65, wm, 1024, bm, bm + 1})


def residue_table(lengths, kb, first=5):
    """every length at a segment start of every residue modulo the 16-byte vector: between two of them lies a filler segment
    of 1 .. 16 / kb keys (a segment like any other: the result has its row).  Returns (offsets, len)."""
    vec = 16 // kb
    off = [first]
    for n in lengths:
        for r in range(vec):
            fill = (r - off[-1]) % vec
            if fill:
                off.append(off[-1] + fill)
            off.append(off[-1] + n)
    return np.array(off, dtype=np.uint64), off[-1] + 3


def table_order(a, offsets, largest=False, key=None):
    """one stable sort of a whole table by (segment, mapped key): (order, segment of each sorted element, its rank inside its
    segment), the order counted from offsets[0]"""
    off = np.asarray(offsets, dtype=np.int64)
    lens = off[1:] - off[:-1]
    lo, hi = int(off[0]), int(off[-1])
    seg = np.repeat(np.arange(len(lens)), lens)
    h, l = T.mapped_limbs(a[lo:hi], key if key else a.dtype.name, largest)
    order = np.lexsort((l, h, seg))                                         # stable: equal keys of a segment in ascending position
    sseg = seg[order]
    return order, sseg, np.arange(hi - lo) - (off[sseg] - lo)


def expected_rows(a, offsets, k, largest, key, out_keys, out_index=None, ordered=None):
    """THE result of a whole table, written into the pre-filled (n_segments, k[, 2]) array `out_keys` (and the (n_segments, k)
    integer array `out_index`): every segment keeps the first k_s of its stable order.  `ordered`: table_order's answer, if
    the caller has it."""
    off = np.asarray(offsets, dtype=np.int64)
    order, sseg, rank = ordered if ordered is not None else table_order(a, offsets, largest, key)
    keep = rank < k
    out_keys[sseg[keep], rank[keep]] = a[int(off[0]):int(off[-1])][order[keep]]
    if out_index is not None:
        out_index[sseg[keep], rank[keep]] = order[keep] - (off[sseg[keep]] - off[0])


def keys_for(n, key, seed, specials=True):
    """n keys with repeats on both sides of any k; floats with their specials, signed types with their extremes"""
    a = T.random_keys(n, key, seed)
    if T.is_wide(key) or n < 8:
        if n > 8:
            a[n // 2:] = a[: n - n // 2]
        return a
    dt = np.dtype(key)
    if specials and dt.kind == "f":
        a = T.float_specials(key, n, seed).copy()
    elif specials and dt.kind == "i":
        a = T.signed_extremes(key, n, seed)
    a[n // 2:] = a[: n - n // 2]
    return a


def shared_digits(n, dtype, j, seed):
    """n keys of `dtype` whose MAPPED keys share their top 12 j bits (clipped to the key's width: all keys equal) and are
    random below: the stream class's select needs more than j levels to tell them apart"""
    a = H.random_bits(n, dtype, seed).copy()
    kb = a.dtype.itemsize
    bits = min(12 * j, 8 * kb)
    if bits == 0:
        return a
    pattern = 0x5AC3F00FA53C0FF0 >> (64 - 8 * kb)
    m = H.set_top(H.mapped_key(a).view(f"i{kb}"), 8 * kb, bits, pattern >> (8 * kb - bits))
    return H.unmapped(m.view(f"u{kb}"), dtype)


def stop_border(dtype, tile, n, extra, seed):
    """n keys (n > tile) and a k: after ONE level of the ascending select c_below + m is tile + extra.  Top digit 1 for
    `below` keys, 2 for m keys (the k-th is among them), 3 for the rest; random below the digit.  Returns (keys, k)."""
    rng = np.random.default_rng(seed)
    kb = np.dtype(dtype).itemsize
    w = 8 * kb
    below = tile // 3
    m = tile + extra - below
    digit = np.full(n, 3, dtype=np.uint64)
    at = rng.permutation(n)
    digit[at[:below]] = 1
    digit[at[below:below + m]] = 2
    low = rng.integers(0, 1 << (w - 12), size=n, dtype=np.uint64)
    keys = H.unmapped(((digit << np.uint64(w - 12)) | low).astype(f"u{kb}"), dtype)
    return keys, below + m // 2


def scattered_ties(dtype, n, tile, seed):
    """n keys: a quarter of a tile below a key T, copies of T at 3 tile / 2 scattered positions, the rest above; and a k whose
    k-th key is T with ties on both sides.  Returns (keys, k, positions of T)."""
    rng = np.random.default_rng(seed)
    kb = np.dtype(dtype).itemsize
    w = 8 * kb
    m = rng.integers(1 << (w - 1), 1 << w, size=n, dtype=np.uint64) | np.uint64(1 << (w - 2))   # above T
    at = rng.permutation(n)
    below, ties = tile // 4, 3 * tile // 2
    m[at[:below]] = rng.integers(0, 1 << (w - 3), size=below, dtype=np.uint64)
    t_at = np.sort(at[below:below + ties])
    m[t_at] = np.uint64(1 << (w - 2))
    return H.unmapped(m.astype(f"u{kb}"), dtype), below + tile // 2, t_at


def mixed_table(wm, bm, seed):
    """one table with all four classes at k <= bm (far: longer than the stream_max the test sets, 3 bm): shuffled, a gap
    before offsets[0], empty segments between, a tail behind the last offset.  Returns (offsets, len, stream_max)."""
    rng = np.random.default_rng(seed)
    lengths = [1, 2, 3, 64, wm, wm - 1, wm + 1, 1025, bm, bm - 1, bm + 1, 2 * bm + 3, 3 * bm, 3 * bm + 1, 4 * bm + 7, 0, 0, 0, 5, wm + 77]
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    off = np.cumsum([3] + lengths).astype(np.uint64)
    return off, int(off[-1]) + 9, 3 * bm
