"""Shared test helpers: an independent numpy statement of the mapped-key order, seeded input
generators shaped like the reference's test inputs (src/test_utils.rs), torch<->numpy glue, and
guard bands around the buffers a test hands the library (Bands / banded)."""
import numpy as np

SEED_C1 = 0x5D570001
SEED_C2 = 0x5D570002
SEED_C3 = 0x5D570003
SEED_C4 = 0x5D570004

DTYPES = ("uint32", "uint64", "int32", "int64", "float32", "float64")
SMALL_DTYPES = ("uint8", "uint16", "int8", "int16")


def uint_view(a):
    return a.view(f"u{a.dtype.itemsize}")


def mapped_key(a):
    """Order-preserving unsigned image of a built-in key type — numpy only, independent of the
    oracle and of the device code (formulae of src/radix_key_impl.rs)."""
    u = uint_view(a)
    w = a.dtype.itemsize * 8
    msb = np.array(1 << (w - 1), dtype=u.dtype)
    if a.dtype.kind == "u":
        return u
    if a.dtype.kind == "i":
        return u ^ msb
    neg = (u >> np.array(w - 1, dtype=u.dtype)) != 0
    return np.where(neg, ~u, u ^ msb)


def reference_sorted(a):
    """THE output of radix_sort_unstable() for a built-in key type: unique because the key map
    is a bijection on the value's bits."""
    order = np.argsort(mapped_key(a), kind="stable")
    return a[order]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(uint_view(a), uint_view(b))


def random_bits(n, dtype, seed):
    """uniform random BIT PATTERNS of the type (floats: NaNs, infs, +-0, denormals all occur,
    like block_rand::<f32> in src/radix_sort.rs:133)"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    u = rng.integers(0, 1 << (8 * dt.itemsize), size=n, dtype=f"u{dt.itemsize}", endpoint=False) \
        if dt.itemsize < 8 else rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)
    return u.view(dt)


def gen_inputs(n, shift, dtype, seed):
    """gen_inputs (src/test_utils.rs:51-61): random, first half >>= shift, second half <<= shift."""
    a = random_bits(n, dtype, seed).copy()
    u = uint_view(a)
    if shift:
        s = np.array(shift, dtype=u.dtype)
        half = n // 2
        if a.dtype.kind == "i":  # Rust >> on iN is arithmetic
            si = a[:half] >> np.array(shift, dtype=a.dtype)
            a[:half] = si
        else:
            u[:half] >>= s
        u[half:] <<= s
    return a


# the 17 lengths of gen_input_set (src/test_utils.rs:63-95), capped for CI time
INPUT_SET_LENGTHS = (0, 1, 10, 100, 5_000, 10_000, 50_000, 100_000, 200_000, 300_000, 500_000, 1_000_000, 2_000_000)


def u32_patterns(seed=7):
    """validate_u32_patterns (src/test_utils.rs:148-262): 4 base inputs x 14 transforms."""
    rng = np.random.default_rng(seed)
    bases = [np.full(128, 0xFFFFFFFF, dtype=np.uint32),
             rng.integers(0, 1 << 32, size=128, dtype=np.uint32),
             rng.integers(0, 1 << 32, size=128_000, dtype=np.uint32),
             rng.integers(0, 1 << 32, size=4, dtype=np.uint32)]
    masks = [0x000000FF, 0x0000FF00, 0x00FF0000, 0xFF000000, 0x00FFFF00, 0xFF0000FF,  # byte-lane masks
             0x80000000, 0x00000001, 0xFFFFFFFE, 0x7FFFFFFF, 0xAAAAAAAA, 0x55555555]
    out = []
    for b in bases:
        for m in masks:
            out.append(b & np.uint32(m))
        out.append(b.copy())
        out.append(np.array([1, 2, 3, 4, 0xFFFFFFFF], dtype=np.uint32))  # the 5-element skew case
    return out


def with_prefixes(n, dtype, prefixes, seed, low_mask=None):
    """random keys whose top 16 bits (of the raw pattern) come from `prefixes`; low bits random & low_mask"""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    w = dt.itemsize * 8
    u = random_bits(n, f"uint{w}", seed).copy()
    if low_mask is not None:
        u &= np.array(low_mask, dtype=u.dtype)
    low = u & np.array((1 << (w - 16)) - 1, dtype=u.dtype)
    top = rng.choice(np.asarray(prefixes, dtype=np.uint64), size=n).astype(u.dtype)
    return (low | (top << np.array(w - 16, dtype=u.dtype))).view(dt)


def giant_buckets_input(rng, dtype):
    """4-byte keys, ~2.35 M: 16-bit prefixes holding 65 536 keys and more — dense and sparse in their low halves, of two
    values, of one value, neighbours in one counter word, the first and the last prefix — among 500 000 random keys"""

    def bucket(prefix, size, kind):
        if kind == "dense":
            low = rng.integers(0, 1 << 16, size=size, dtype=np.uint32)
        elif kind == "sparse":      # few distinct values far apart: long empty stretches of the count table
            low = rng.choice(np.array([0, 1, 300, 30000, 32767, 32768, 65000, 65535], dtype=np.uint32), size=size)
        elif kind == "two":
            low = rng.choice(np.array([0, 65535], dtype=np.uint32), size=size)
        elif kind == "one":
            low = np.full(size, 0x8000, dtype=np.uint32)
        else:                        # "narrow": every value of a small range, many times
            low = rng.integers(1000, 1100, size=size, dtype=np.uint32)
        return low | np.uint32(prefix << 16)

    parts = [bucket(0x0000, 65_536, "dense"), bucket(0xFFFF, 70_001, "sparse"), bucket(0x1234, 300_000, "dense"),
             bucket(0x1235, 65_537, "two"), bucket(0x8000, 131_072, "one"), bucket(0x7FFF, 1_100_000, "narrow"),
             bucket(0x4000, 65_535, "dense"), bucket(0x4001, 20_000, "two"), random_bits(500_000, "uint32", seed=5)]
    a = np.concatenate(parts)
    rng.shuffle(a)
    return a.view(dtype)


def heavy_digit_inputs(n, dtype, level, seed):
    """inputs that put the lr variants of out_of_place_sort to work (src/sorts/out_of_place_sort.rs:202-389: a
    bucket written from both ends when many equal digits sit next to each other) and the heavy-digit ranking of K3"""
    rng = np.random.default_rng(seed)
    w = np.dtype(dtype).itemsize * 8
    ut = f"uint{w}"
    base = random_bits(n, ut, seed).copy()
    sh = np.array(8 * level, dtype=ut)
    clear = ~(np.array(0xFF, dtype=ut) << sh)

    def with_digits(d):
        return ((base & clear) | (d.astype(ut) << sh)).view(dtype)

    out = {}
    d = rng.integers(0, 256, size=n)
    d[rng.random(n) < 0.9] = 0x5A
    out["90% one digit"] = with_digits(d)
    out["two digits only"] = with_digits(rng.choice([3, 200], size=n))
    out["one digit per 64-key round"] = with_digits(np.repeat(rng.integers(0, 256, size=(n + 63) // 64), 64)[:n])
    out["sorted by digit"] = with_digits(np.sort(rng.integers(0, 256, size=n)))
    out["long equal runs"] = with_digits(np.repeat(rng.integers(0, 256, size=(n + 999) // 1000), 1000)[:n])
    return out


def to_device(a):
    import torch
    t = torch.from_numpy(a.view({1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]).copy()).cuda()
    return t.view(getattr(torch, a.dtype.name))


def to_host(t, dtype):
    import torch
    it = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[np.dtype(dtype).itemsize]
    return t.view(it).cpu().numpy().view(dtype)


# ---- guard bands: where the library reads and writes ------------------------------------------------------------

BAND_BYTES = 256 << 10  # each side: more than one tile of any scatter or K4 shape (at most 21 504 x 8 bytes)


def poison_pattern(key):
    """the bytes of the smallest mapped key of `key` (a numpy dtype name, "u128" or "bytes"): 0 for unsigned keys and byte
    strings, MIN for signed ones, all ones for floats (the negative NaN with the largest payload)"""
    if key in ("u128", "bytes"):
        return np.zeros(16 if key == "u128" else 1, dtype=np.uint8)
    dt = np.dtype(key)
    w = dt.itemsize * 8
    bits = 0 if dt.kind == "u" else (1 << (w - 1)) if dt.kind == "i" else (1 << w) - 1
    return np.array([bits], dtype=f"<u{dt.itemsize}").view(np.uint8)


def without_poison(a, key=None):
    """a copy of `a` in which every occurrence of the poison key is replaced by a key that differs in its lowest bit, so
    that a poison key in a result can only have come from a band"""
    a = np.array(a, copy=True)
    if key in ("bytes", "u128"):          # (n, N) uint8 rows / (n, 2) uint64 limbs [low, high]: the all-zero rows
        zero = ~a.any(axis=1)
        a[zero, 0 if key == "u128" else -1] = 1
        return a
    u = uint_view(a)
    p = poison_pattern(a.dtype.name).view(u.dtype)[0]
    u[u == p] ^= u.dtype.type(1)
    return a


def _align_up(x, a):
    return -(-x // a) * a


class Bands:
    """One allocation that holds one or more views, with bands of known bytes everywhere else: ``band_bytes`` before the
    first view, at least ``band_bytes`` after the last one, and the gaps between views.  ``parts``: (name, init, gap) —
    ``init`` a numpy array (the view's contents, shape and type) or a (shape, dtype) pair (the view then holds the fill
    too); ``gap``: the view starts that many bytes after the previous view's end (the first: after the leading band), so
    the allocation's 256-byte alignment makes the first view's address ``gap`` modulo 256.  No view ends flush with the
    allocation: a stray access lands in a band, never past the buffer.  ``fill``: "random" (seeded bytes: catches writes)
    or a pattern from :func:`poison_pattern` (catches band elements read and used as keys).  ``device``: a torch device,
    or None for a numpy buffer (the host entry points).  :meth:`check` compares every byte outside the views with the
    image saved at construction."""

    def __init__(self, parts, band_bytes=BAND_BYTES, seed=0, fill="random", device="cuda"):
        assert band_bytes % 256 == 0 and band_bytes > 0
        self.device = device
        self.spans = []   # (name, start, end, shape, dtype)
        pos = band_bytes
        for name, init, gap in parts:
            if isinstance(init, np.ndarray):
                shape, dtype = init.shape, init.dtype
            else:
                shape, dtype = tuple(int(x) for x in np.atleast_1d(init[0])), np.dtype(init[1])
            start = pos + gap
            nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
            self.spans.append((name, start, start + nbytes, shape, dtype))
            pos = start + nbytes
        total = _align_up(pos, 256) + band_bytes
        if isinstance(fill, str):
            assert fill == "random", fill
            img = np.random.default_rng(seed).integers(0, 256, size=total, dtype=np.uint8)
        else:
            img = np.resize(np.asarray(fill, dtype=np.uint8), total)   # the pattern repeats from the allocation's start
        for (_name, start, end, _shape, _dtype), (_n, init, _gap) in zip(self.spans, parts):
            if isinstance(init, np.ndarray):
                img[start:end] = np.ascontiguousarray(init).reshape(-1).view(np.uint8)
        self.image = img
        if device is None:
            host = np.empty(total + 256, dtype=np.uint8)               # numpy: start on a 256-byte boundary as well
            base = (-host.ctypes.data) % 256
            self.raw = host[base:base + total]
            self.raw[:] = img
        else:
            import torch
            self.raw = torch.from_numpy(img.copy()).to(device)         # (a copy: never the saved image's memory)
        self.views = {name: self._view(start, end, shape, dtype) for name, start, end, shape, dtype in self.spans}

    def _view(self, start, end, shape, dtype):
        piece = self.raw[start:end]
        if self.device is None:
            return piece.view(dtype).reshape(shape)
        import torch
        return piece.view(getattr(torch, dtype.name)).view(shape)

    def __getitem__(self, name):
        return self.views[name]

    def span(self, name):
        for s in self.spans:
            if s[0] == name:
                return s
        raise KeyError(name)

    def extended(self, name, extra_bytes):
        """the 1-D view `name` grown by `extra_bytes` into the band behind it (a buffer handed over with more elements than
        the call needs: what lies past len is still checked as a band)"""
        _n, start, end, _shape, dtype = self.span(name)
        nxt = [s[1] for s in self.spans if s[1] >= end and s[0] != name]
        assert extra_bytes % dtype.itemsize == 0 and end + extra_bytes < (min(nxt) if nxt else self.image.size)
        return self._view(start, end + extra_bytes, ((end + extra_bytes - start) // dtype.itemsize,), dtype)

    def _bytes(self, a, b):
        if self.device is None:
            return np.array(self.raw[a:b])
        return self.raw[a:b].cpu().numpy()

    def changes(self, untouched=()):
        """descriptions of what changed: in every band and gap, and in the views named in `untouched`"""
        out = []
        edges = [0] + [x for s in self.spans for x in (s[1], s[2])] + [self.image.size]
        for i in range(0, len(edges), 2):        # the regions outside the views
            a, b = edges[i], edges[i + 1]
            diff = np.flatnonzero(self._bytes(a, b) != self.image[a:b])
            if diff.size == 0:
                continue
            lo, hi = a + int(diff[0]), a + int(diff[-1]) + 1
            if i == 0:
                name, s0 = self.spans[0][0], self.spans[0][1]
                out.append(f"bytes [-{s0 - lo}, -{s0 - hi}) before {name}[0] changed ({diff.size} differ)")
            else:
                name, e = self.spans[i // 2 - 1][0], self.spans[i // 2 - 1][2]
                out.append(f"bytes [+{lo - e}, +{hi - e}) after {name}[len) changed ({diff.size} differ)")
        for name in untouched:
            _n, a, b, _shape, _dtype = self.span(name)
            diff = np.flatnonzero(self._bytes(a, b) != self.image[a:b])
            if diff.size:
                out.append(f"bytes [{int(diff[0])}, {int(diff[-1]) + 1}) of {name}, which must stay untouched, changed "
                           f"({diff.size} differ)")
        return out

    def check(self, what="", untouched=()):
        """raise AssertionError naming the first and last changed byte of every band (and untouched view) that changed"""
        bad = self.changes(untouched)
        assert not bad, f"{what}: " + "; ".join(bad)


def banded(n, dtype, offset_bytes=0, band_bytes=BAND_BYTES, seed=0, fill="random", device="cuda", init=None, name="keys"):
    """One view of `n` elements of `dtype` (``n`` a tuple for rows), `offset_bytes` after a band of `band_bytes` and with a
    band behind it; ``init``: its contents (else the fill).  Returns the :class:`Bands`: ``bands[name]`` is the view,
    ``bands.check()`` the test."""
    return Bands([(name, init if init is not None else (n, dtype), offset_bytes)], band_bytes, seed, fill, device)


# ---- the key sample (presample_kernel) restated, and inputs built around its positions ---------------------------------
# Every constant below is the library's own, quoted from rdst_amd/csrc/rdst_kernels.hip (the line it stands on):
PRESAMPLE_KEYS = 8192            # :452  keys the sample reads, at the positions k * (n / 8192)
PRESAMPLE_MIN_LEN = 1 << 26      # :453  no sample below this length
PRESAMPLE_DUP_LIMIT = 5000       # :458  repeated low halves (4-byte keys)
PRESAMPLE_TOP_LIMIT = 2 * PRESAMPLE_KEYS // 256   # :459  hits on one top byte: 64
GIANT_MIN = 65536                # :760
EXPAND_MAX = 65535               # :2862
GIANT_MAX = 4096                 # :4481
LOCAL_TILE = {4: 12 * 64 * 22, 8: 16 * 64 * 16}   # :2310-2312  local_tile(): K4's tile, 16 896 / 16 384 keys
MSD_WAVES, MSD_KPT = 12, {4: 22, 8: 11}           # :4451-4461  pass A's block and keys per thread
SAMPLE_WORDS = ("win_shift", "win_top", "gross_skew", "top_skew", "low_dups", "predict_lsd")

_ROUTE_FIELDS = dict(hybrid=True, count_sort=True, halves=True, presample=True, wide2=True, wide3=True, atomic_route=True,
                     exact_msd=True, giants=True, chain_routes=True, expand=True, atomic_wide=True, split=True,
                     split_always=False, predict=True)                 # :4359-4375  RouteTuning's defaults
_ROUTE_MODES = {7: (False, None), 0: (False, ("hybrid", False)), 1: (True, None), 2: (False, ("count_sort", False)),
                3: (False, ("halves", False)), 5: (False, ("presample", False)), 6: (False, ("wide2", False)),
                8: (True, ("atomic_wide", False)), 9: (False, ("expand", False)), 10: (True, ("chain_routes", False)),
                11: (True, ("giants", False)), 12: (True, ("exact_msd", False)), 14: (True, ("predict", False)),
                15: (True, ("wide3", False)), 16: (True, ("split", False)), 17: (True, ("split_always", True))}   # :4400-4417


def route_tuning(mode=1, min_len=0):
    """what rdst_hip_set_hybrid(mode, min_len) leaves in force: kRouteModes' preset (the default with or without the atomic
    route, at most one field changed) and the length knob"""
    atomic, change = _ROUTE_MODES[int(mode)]
    t = dict(_ROUTE_FIELDS, atomic_route=atomic, min_len=int(min_len), mode=int(mode))
    if change:
        t[change[0]] = change[1]
    return t


def routes_tried(n, key_bytes, t):
    """(try_atomic, try_hybrid) of a whole key-only sort: atomic_eligible, hybrid_eligible, pick_routes (:4642-4657, :5007-5016);
    4-byte keys below 2^30 bytes of slice (pass shape 4, halves possible) are assumed, as every test here has them"""
    amin = t["min_len"] or ((1 << 26) if key_bytes == 8 else (3 << 26))
    hmin = t["min_len"] or (1 << 28)
    mean = n / 65536
    atomic = t["hybrid"] and t["atomic_route"] and amin <= n < (1 << 30) and mean + 8.0 * mean ** 0.5 <= LOCAL_TILE[key_bytes]
    if key_bytes == 4:
        assert n * 4 < (1 << 32)
    else:
        atomic = atomic and t["atomic_wide"] and t["count_sort"] and t["wide2"]
    cap = EXPAND_MAX if key_bytes == 4 and t["count_sort"] and t["expand"] else LOCAL_TILE[key_bytes]
    hybrid = t["hybrid"] and hmin <= n <= 65536 * cap and n < (1 << 32)
    hybrid = hybrid and (not atomic or (t["chain_routes"] and (key_bytes == 8 or (t["halves"] and t["count_sort"]))))
    return bool(atomic), bool(hybrid)


def sample_positions(n):
    return np.arange(PRESAMPLE_KEYS, dtype=np.int64) * (n // PRESAMPLE_KEYS)


def unmapped(m, dtype):
    """inverse of mapped_key: the keys of `dtype` whose mapped images are the unsigned integers `m`"""
    dt = np.dtype(dtype)
    w = dt.itemsize * 8
    m = np.asarray(m, dtype=f"u{dt.itemsize}")
    msb = np.array(1 << (w - 1), dtype=m.dtype)
    if dt.kind == "u":
        u = m.copy()
    elif dt.kind == "i":
        u = m ^ msb
    else:                       # a mapped float with its top bit set was a non-negative one (u ^ msb), else a negative (~u)
        u = np.where((m & msb) != 0, m ^ msb, ~m)
    return u.view(dt)


def sample_verdict(keys, route_tuning=None, n=None):
    """The six plan words presample_kernel / launch_presample (:461-546, :4793-4805) leave for this slice, from numpy alone.
    `keys`: the whole slice, or (with `n`) just its 8 192 keys at sample_positions(n), in that order."""
    t = route_tuning or globals()["route_tuning"]()
    if n is None:
        n = len(keys)
        keys = keys[sample_positions(n)] if n >= PRESAMPLE_KEYS else keys
    out = dict.fromkeys(SAMPLE_WORDS, 0)
    kb = keys.dtype.itemsize
    if not t["presample"] or n < PRESAMPLE_MIN_LEN or not any(routes_tried(n, kb, t)):
        return out
    assert len(keys) == PRESAMPLE_KEYS
    w = kb * 8
    m = mapped_key(keys).astype(np.uint64)
    top16 = m >> np.uint64(w - 16)
    diff = int(np.bitwise_and.reduce(top16) ^ np.bitwise_or.reduce(top16)) & 0xFFFF
    lead = 16 - diff.bit_length()                       # clz(diff) - 16 for a 16-bit diff; 16 when the prefixes agree
    ws = min(8, lead)
    out["win_shift"] = ws
    out["win_top"] = int(np.bitwise_or.reduce(top16)) >> (16 - ws) if ws else 0
    b = ((m >> np.uint64(w - 16 - ws)) & np.uint64(0xFFFF)).astype(np.int64)
    limit = 12 + 4 * LOCAL_TILE[kb] * PRESAMPLE_KEYS // n
    assert limit <= 64
    # (8-bit counters: one that reaches the limit raises the flag before it could carry, and a carry only ever raises a
    # neighbour's count while the flag is already up — the flag needs no model of the wrap)
    out["gross_skew"] = int(np.bincount(b, minlength=65536).max() >= limit)
    hits = np.bincount(b >> 8, minlength=256)           # (32-bit counters)
    out["top_skew"] = int(hits.max() >= PRESAMPLE_TOP_LIMIT)
    est = n * hits.astype(object) // (PRESAMPLE_KEYS * 256)
    if kb == 4:
        mult = np.bincount((m & np.uint64(0xFFFF)).astype(np.int64), minlength=65536)
        dups = int((mult[mult > 0] - 1).sum())
        # a low half seen 256 times wraps its 8-bit counter (one hit in 256 then counts as new, a carry may make a neighbour's
        # first hit count as seen): at most 32 either way over 8 192 samples — the restatement stays away from that margin
        assert mult.max() < 256 or abs(dups - PRESAMPLE_DUP_LIMIT) > 64, "low halves wrap next to the limit: not modelled"
        out["low_dups"] = int(dups >= PRESAMPLE_DUP_LIMIT)
        big4 = t["count_sort"] and t["expand"] and t["predict"]
        giant_min = GIANT_MIN if big4 else 0
        giant_max = GIANT_MAX if big4 and t["giants"] and n < (1 << 30) else 0
        looks_giant = sum(1 for h, e in zip(hits, est) if giant_min and h >= 8 and e >= giant_min + giant_min // 4)
        out["predict_lsd"] = int(bool(giant_min) and looks_giant * 256 > giant_max + giant_max // 2)
    else:
        cap = LOCAL_TILE[8] if t["predict"] else 0
        out["predict_lsd"] = int(any(cap and h >= 16 and e > 2 * cap for h, e in zip(hits, est)))
    return out


def predicted_route(verdict, n, key_bytes, t, atomic_ok, giants16, bmax16):
    """The route the code must end on (run_pipeline's kernels, each looking at the plan: msd_scatter_kernel :1856-1864,
    msd_finish_kernel :949-960, hist16_kernel :578-585, route_kernel :777-783 and :846).  `atomic_ok`: would the atomic route's own
    checks pass (every key inside the window, no area or slot over its room)?  None when the test cannot tell.  `giants16`,
    `bmax16`: how many 16-bit prefixes of the mapped keys hold 65 536 keys and more, and the largest prefix count.  Returns None
    where the inputs leave it open."""
    try_atomic, try_hybrid = routes_tried(n, key_bytes, t)
    flagged = verdict["gross_skew"] or verdict["top_skew"] or verdict["predict_lsd"]
    if try_atomic and not flagged:
        if atomic_ok is None:
            return None
        if atomic_ok:
            return "atomic"
    if not try_hybrid or verdict["predict_lsd"]:
        return "lsd"
    giants = key_bytes == 4 and t["giants"] and t["count_sort"] and t["expand"] and n < (1 << 30)
    if giants:
        return "hybrid" if giants16 <= GIANT_MAX else "lsd"
    cap = EXPAND_MAX if key_bytes == 4 and t["count_sort"] and t["expand"] else LOCAL_TILE[key_bytes]
    return "hybrid" if bmax16 <= cap and not verdict["gross_skew"] else "lsd"


def pass_a_geometry(key_bytes):
    """pass A of the atomic route (msd_scatter_kernel as atomic_stage launches it, :5152): keys per thread, the keys one wave
    covers (index order inside a tile is wave, round, lane) and the tile"""
    kpt = MSD_KPT[key_bytes]
    return {"kpt": kpt, "span": 64 * kpt, "tile": MSD_WAVES * 64 * kpt}


# Builders.  They work on torch tensors (any device) that hold MAPPED keys as the bits of int32 / int64 — the space in which the
# window and the prefixes live — and `unmapped_bits` turns such a tensor into the bit patterns of the key type.

def _signed(x, w):
    x &= (1 << w) - 1
    return x - (1 << w) if x >> (w - 1) else x


def rand_mapped(torch, n, w, gen, device):
    """uniform random bits (one pattern of 2^w never occurs: randint's upper bound is exclusive)"""
    it = torch.int32 if w == 32 else torch.int64
    info = torch.iinfo(it)
    return torch.randint(info.min, info.max, (n,), dtype=it, device=device, generator=gen)


def set_top(m, w, nbits, value):
    """m with its top `nbits` bits replaced by `value` (a Python int or a tensor of m's type)"""
    if nbits == 0:
        return m
    low = m & _signed((1 << (w - nbits)) - 1, w)
    if isinstance(value, int):
        return low | _signed(value << (w - nbits), w)
    return low | (value << (w - nbits))


def top_bits(m, w, nbits):
    """the top `nbits` bits of every key, as non-negative int64"""
    return (m.long() >> (w - nbits)) & ((1 << nbits) - 1)


def unmapped_bits(torch, m, name):
    """the bits of the keys of type `name` whose mapped images are the bits `m` (torch twin of unmapped)"""
    kind = np.dtype(name).kind
    mn = torch.iinfo(m.dtype).min
    if kind == "u":
        return m.clone()
    if kind == "i":
        return m ^ mn
    return torch.where(m < 0, m ^ mn, ~m)


def sample_index(torch, n, device):
    return torch.arange(PRESAMPLE_KEYS, device=device, dtype=torch.int64) * (n // PRESAMPLE_KEYS)


def plant(keys, positions, values):
    """keys with `values` at `positions` (in place; returns keys)"""
    keys[positions] = values
    return keys


def with_sample(torch, rest, sampled):
    """`rest` with the 8 192 keys `sampled` at the sample's positions"""
    return plant(rest, sample_index(torch, rest.numel(), rest.device), sampled)


def not_sampled(n, positions):
    """the positions, checked: none of them is one the sample reads"""
    step = n // PRESAMPLE_KEYS
    for p in positions:
        assert 0 <= p < n and (p % step != 0 or p // step >= PRESAMPLE_KEYS), (n, p)
    return list(positions)


def window_pattern(kind, d):
    """the shared top `d` bits: all zeros, all ones, or mixed (0b1011010010110100 cut to d bits)"""
    return {"zeros": 0, "ones": (1 << d) - 1, "mixed": 0xB4B4 >> (16 - d)}[kind] if d else 0


def window_keys(torch, n, w, d, pattern, gen, device):
    """random mapped keys that share exactly their top d bits (value `pattern`): the bit below takes both values among the
    SAMPLED keys (d < 16)"""
    m = set_top(rand_mapped(torch, n, w, gen, device), w, d, pattern)
    if d < 16:
        pos = sample_index(torch, n, device)[:2]
        two = set_top(m[pos], w, d + 1, torch.tensor([pattern << 1, (pattern << 1) | 1], device=device, dtype=m.dtype))
        plant(m, pos, two)
    return m


def spread_sample(torch, w, gen, device):
    """8 192 mapped keys a truthful uniform slice could show: the 16-bit prefixes 8 k (distinct, 32 on every top byte), random
    bits below"""
    m = rand_mapped(torch, PRESAMPLE_KEYS, w, gen, device)
    return set_top(m, w, 16, torch.arange(PRESAMPLE_KEYS, device=device, dtype=m.dtype) * 8)


def gross_sample(torch, w, hits, gen, device, prefix=0xF008):
    """spread_sample with `hits` keys on one 16-bit prefix: its own holder and one key each from the top bytes 0, 1, ... (so
    the prefix's top byte gains hits - 1 < 64 - 32)"""
    assert prefix % 8 == 0 and 1 <= hits <= 30 < (prefix >> 8)
    m = spread_sample(torch, w, gen, device)
    idx = torch.arange(hits - 1, device=device) * 32 + 1      # sample 32 j + 1 holds prefix 8 (32 j + 1): top byte j
    m[idx] = set_top(m[idx], w, 16, prefix)
    return m


def top_sample(torch, w, hits, gen, device, byte=0x47):
    """spread_sample with `hits` keys on one top byte, on distinct prefixes (no prefix is hit twice)"""
    assert 32 <= hits <= 32 + 224
    m = spread_sample(torch, w, gen, device)
    extra = hits - 32
    donors = [j for j in range(256) if j != byte][:extra]
    idx = torch.tensor([32 * j + 1 for j in donors], device=device, dtype=torch.int64)
    pref = torch.tensor([(byte << 8) | (8 * (k % 32) + 1 + k // 32) for k in range(extra)], device=device, dtype=m.dtype)
    if extra:
        m[idx] = set_top(m[idx], w, 16, pref)
    return m


def dups_sample(torch, dups, gen, device):
    """spread_sample (4-byte keys) whose low halves take 8 192 - dups distinct values, each at most a few times"""
    m = spread_sample(torch, 32, gen, device)
    distinct = PRESAMPLE_KEYS - dups
    assert 64 <= distinct <= PRESAMPLE_KEYS and 20 * distinct + 3 < 65536
    low = (torch.arange(PRESAMPLE_KEYS, device=device, dtype=torch.int64) % distinct) * 20 + 3
    return (m & _signed(0xFFFF0000, 32)) | low.to(m.dtype)


def bytes_sample(torch, w, nbytes, hits, gen, device):
    """8 192 mapped keys with `hits` on each of the top bytes 16, 24, ... (`nbytes` of them), the rest dealt round over all
    other top bytes; prefixes inside a byte as even as they can be"""
    heavy = nbytes * hits
    assert heavy <= PRESAMPLE_KEYS and nbytes <= 30
    m = rand_mapped(torch, PRESAMPLE_KEYS, w, gen, device)
    k = torch.arange(PRESAMPLE_KEYS, device=device, dtype=torch.int64)
    hp = ((16 + 8 * (k // hits)) << 8) | ((k % hits) * 256 // hits)
    others = torch.tensor([b for b in range(256) if not (b % 8 == 0 and 16 <= b < 16 + 8 * nbytes)], device=device, dtype=torch.int64)
    rest = (k - heavy).clamp(min=0)
    op = (others[rest % others.numel()] << 8) | ((rest // others.numel()) * 8 % 256 + 3)
    return set_top(m, w, 16, torch.where(k < heavy, hp, op).to(m.dtype))


def bytes_population(torch, m, w, nbytes, hits):
    """m (in place) with the share hits / 8 192 of its keys, spread evenly, on each of the top bytes bytes_sample makes heavy"""
    i = torch.arange(m.numel(), device=m.device, dtype=torch.int64) % PRESAMPLE_KEYS
    on = i < nbytes * hits
    byte = (16 + 8 * (i // hits)).to(m.dtype)
    m[on] = set_top(m[on], w, 8, byte[on])
    return m


def increasing_keys(torch, n, w, gen, device, below_bits=None, dense_from=None):
    """strictly increasing mapped keys: key i = i * K + r_i with r_i random below K = floor(range / n) — over the whole
    range, below 2^below_bits, or (dense_from) the ids dense_from + i"""
    it = torch.int32 if w == 32 else torch.int64
    i = torch.arange(n, device=device, dtype=torch.int64)
    if dense_from is not None:
        v = i + dense_from
    else:
        bits = below_bits or w
        k = (1 << bits) // n
        assert k >= 2
        if bits == 64:      # i * K + r - 2^63 stays inside int64; adding 2^63 back is a flip of the top bit
            v = (i * k + torch.randint(0, k, (n,), device=device, generator=gen) + torch.iinfo(torch.int64).min) ^ torch.iinfo(torch.int64).min
        else:
            v = i * k + torch.randint(0, k, (n,), device=device, generator=gen)
    if w == 32:
        v = torch.where(v >= (1 << 31), v - (1 << 32), v).to(it)
    return v


def swap_spots(n, key_bytes):
    """where pass A's own per-key checks have their borders: lanes, a wave's span, the tile, the last (partial) tile"""
    g = pass_a_geometry(key_bytes)
    span, tile = g["span"], g["tile"]
    mid, last = tile * (n // tile // 2), tile * (n // tile)
    spots = [0, 62, 63, 64, span - 2, span - 1, span, tile - 2, tile - 1, tile, tile + span - 1, mid - 2, mid - 1, mid, mid + 1,
             last - 2, last - 1, last, n - 3, n - 2]
    if last + 1 < n - 1:
        spots.append(last + 1)
    assert all(0 <= s < n - 1 for s in spots)
    return sorted(set(spots))


def stray_positions(n, key_bytes):
    """where a key outside the window hides: the first tile, both sides of its border, the middle, the last full tile's last
    key, the partial tile's last key, and the first tile of each of the eight XCDs (blocks 0..7) — none of them sampled"""
    tile = pass_a_geometry(key_bytes)["tile"]
    assert n % tile != 0
    pos = [1, tile - 1, tile, n // 2 + 1, tile * (n // tile) - 1, n - 1] + [b * tile + 777 for b in range(8)]
    return not_sampled(n, pos)


# ---- key-value sorts: the pair tile, values that name their position, the reference, and the inputs of the pairs tests ------

PAIR_THREADS = 768               # :4970  PAIR_WAVES = 12 waves of 64 lanes
PAIR_KPT = {8: 11, 12: 7, 16: 5}  # :4969  constexpr int pair_kpt(size_t key_bytes, size_t val_bytes) { return key_bytes + val_bytes <= 8 ? 11 : (key_bytes + val_bytes <= 12 ? 7 : 5); }
PAIR_WIDTHS = ((4, 4), (4, 8), (8, 4), (8, 8))
VALUE_ODD = {4: 0x9E3779B1, 8: 0x9E3779B97F4A7C15}


def pair_kpt(key_bytes, val_bytes):
    return PAIR_KPT[key_bytes + val_bytes]


def pair_tile(key_bytes, val_bytes):
    """pairs per tile of launch_pass_pairs: 8 448, 5 376 or 3 840"""
    return PAIR_THREADS * pair_kpt(key_bytes, val_bytes)


def pair_lengths(key_bytes, val_bytes):
    """a few tiles with a single pair in the last one; several tiles on every one of the 8 chains and a partial last tile"""
    t = pair_tile(key_bytes, val_bytes)
    return 3 * t + 1, 37 * t + t // 2 + 3


def key_dtype(key_bytes, kind):
    """numpy dtype name of a `key_bytes`-wide key of kind "u", "i" or "f" """
    return {"u": "uint", "i": "int", "f": "float"}[kind] + str(8 * key_bytes)


def position_values(n, vdtype):
    """value i = i * an odd constant modulo 2^w: a bijection of the index, so a value names the position it came from, and
    every bit of the value is in play"""
    dt = np.dtype(vdtype)
    ut = np.dtype(f"u{dt.itemsize}")
    return (np.arange(n, dtype=ut) * ut.type(VALUE_ODD[dt.itemsize])).view(dt)


def value_positions(vals):
    """inverse of position_values: the positions the values came from (int64)"""
    w = vals.dtype.itemsize
    ut = np.dtype(f"u{w}")
    inv = pow(VALUE_ODD[w], -1, 1 << (8 * w))
    return (uint_view(vals) * ut.type(inv)).astype(np.int64)


def expected_pairs(keys, vals):
    """THE output of a stable key-value sort: the stable order of the mapped keys is the single permitted one"""
    order = np.argsort(mapped_key(keys), kind="stable")
    return keys[order], vals[order]


def keys_with_constant_levels(n, dtype, levels, seed, digit=0x5A):
    """random keys whose MAPPED bytes at `levels` all hold `digit` (built in mapped space: a constant raw byte of a float is
    not constant once the negatives are complemented); every other level stays random"""
    dt = np.dtype(dtype)
    m = uint_view(random_bits(n, f"uint{8 * dt.itemsize}", seed).copy())
    for l in levels:
        sh = np.array(8 * l, dtype=m.dtype)
        m = (m & ~(np.array(0xFF, dtype=m.dtype) << sh)) | (np.array(digit, dtype=m.dtype) << sh)
    return unmapped(m, dtype)


def constant_levels(keys):
    """the set of levels at which the mapped digit of `keys` takes one value (the levels a sort with level skipping skips)"""
    m = mapped_key(keys)
    out = set()
    for l in range(keys.dtype.itemsize):
        d = (m >> np.array(8 * l, dtype=m.dtype)) & np.array(0xFF, dtype=m.dtype)
        if (d == d[0]).all():
            out.add(l)
    return out


def constant_level_sets(key_bytes):
    """the level sets of the skipped-level cases: (name, levels, passes left)"""
    top, mid = key_bytes - 1, {4: 1, 8: 3}[key_bytes]
    every = set(range(key_bytes))
    sets = [("level 0", {0}), ("level 1", {1}), ("top level", {top})]
    if key_bytes == 8:
        sets.append(("a middle level", {mid}))
    sets += [("levels 0 and 1", {0, 1}), ("level 0 and top", {0, top}), ("all but level 0", every - {0}),
             ("all but the top", every - {top}), ("all but a middle level", every - {mid}), ("none", set())]
    return [(f"{name} constant", levels, key_bytes - len(levels)) for name, levels in sets]


def constant_level_inputs(key_bytes, val_bytes, kind):
    """(name, levels, passes, keys) of every skipped-level case of the pairs tests, at both pair lengths: `levels` the
    constant ones, `passes` the number left to execute.  Float keys: one more case whose keys share one sign (the top level
    stays busy, but on half of its digits)"""
    dtype = key_dtype(key_bytes, kind)
    for j, n in enumerate(pair_lengths(key_bytes, val_bytes)):
        for i, (name, levels, passes) in enumerate(constant_level_sets(key_bytes)):
            yield f"{name}, n={n}", levels, passes, keys_with_constant_levels(n, dtype, sorted(levels), seed=9000 + 100 * j + i)
        if kind == "f":
            m = uint_view(random_bits(n, f"uint{8 * key_bytes}", seed=9090 + j).copy())
            m |= np.array(1 << (8 * key_bytes - 1), dtype=m.dtype)   # mapped top bit set: the non-negative floats
            yield f"one sign, n={n}", set(), key_bytes, unmapped(m, dtype)


COPY_BACK_LEVELS = {1}   # level 1 constant: 3 or 7 passes, the result ends in the tmps


def copy_back_inputs(key_bytes, val_bytes):
    """the keys of the copy-back tests: level 1 constant (an odd number of passes) at four consecutive lengths from the
    short pair length, so that n * sizeof(V) leaves every remainder modulo 16 a value width allows"""
    n0 = pair_lengths(key_bytes, val_bytes)[0]
    for r in range(4):
        yield keys_with_constant_levels(n0 + r, key_dtype(key_bytes, "u"), sorted(COPY_BACK_LEVELS), seed=9500 + r)


def mask_other_bytes(a, level):
    """`a` with every byte but the one at `level` cut to its two low bits: many whole keys are equal"""
    u = uint_view(a)
    mask = sum((0xFF if b == level else 0x03) << (8 * b) for b in range(u.dtype.itemsize))
    return (u & np.array(mask, dtype=u.dtype)).view(a.dtype)


def pair_digit_levels(key_bytes):
    return 0, 1, key_bytes - 1


def pair_heavy_digit_inputs(key_bytes, val_bytes):
    """(name, level, keys) of heavy_digit_inputs at pair sizes: unsigned keys, both pair lengths, the levels 0, 1 and top"""
    dtype = key_dtype(key_bytes, "u")
    for n in pair_lengths(key_bytes, val_bytes):
        for level in pair_digit_levels(key_bytes):
            for name, a in heavy_digit_inputs(n, dtype, level, seed=n + level).items():
                yield name, level, a


def increasing_mapped(n, dtype, seed):
    """strictly increasing keys (in mapped order) with every level busy: mapped key i = i * K + r_i, r_i random below K"""
    w = 8 * np.dtype(dtype).itemsize
    k = (1 << w) // n
    assert k >= 2
    r = np.random.default_rng(seed).integers(0, k, size=n, dtype=np.uint64)
    return unmapped((np.arange(n, dtype=np.uint64) * np.uint64(k) + r).astype(f"u{w // 8}"), dtype)


def chain_split_cases(n, dtype, seed=77, short=40_000, tiny=700):
    """inputs that bend the split of a pass's source into 8 chain segments (unsigned bit patterns of the width of `dtype`): a
    skipped middle level, previous digits crowded into one group or missing from most, segments shorter than a tile"""
    u = np.dtype(f"uint{8 * np.dtype(dtype).itemsize}")
    bits = u.itemsize * 8
    rng = np.random.default_rng(seed)
    full = rng.integers(0, 1 << 63, size=n, dtype=np.uint64).astype(u) if bits == 32 else rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    return {
        "level 1 constant": (full & ~u.type(0xFF00)) | u.type(0x4200),
        "level 0 in one group": (full & ~u.type(0xE0)),
        "level 0 90% in group 7": np.where(rng.random(n) < 0.9, full | u.type(0xE0), full),
        "level 1 only two digits": (full & ~u.type(0xFE00)),
        "levels 0-1 constant": (full & ~u.type(0xFFFF)) | u.type(0x1234),
        "top levels only": full & (u.type(0xFF) << u.type(bits - 8)),
        "uniform": full,
        "short": full[:short],
        "tiny": full[:tiny],
    }
