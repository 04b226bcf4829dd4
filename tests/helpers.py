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


def heavy_digit_inputs(n, dtype, level, seed, run=1000):
    """inputs that put the lr variants of out_of_place_sort to work (src/sorts/out_of_place_sort.rs:202-389: a
    bucket written from both ends when many equal digits sit next to each other) and the heavy-digit ranking of K3;
    `run`: the length of the "long equal runs" """
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
    out["long equal runs"] = with_digits(np.repeat(rng.integers(0, 256, size=(n + run - 1) // run), run)[:n])
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


# ---- 16-byte keys ("u128" / "i128"): (n, 2) uint64 rows of limbs [low, high]; level l is byte l % 8 of limb l // 8 -------------

def is_wide(key):
    return key in ("u128", "i128")


def wide_mapped(a, key):
    """the limbs of the mapped keys: the top bit of `high` flipped for "i128" (its own inverse: mapped limbs -> keys too)"""
    m = np.array(a, dtype=np.uint64, copy=True)
    if key == "i128":
        m[:, 1] ^= np.uint64(1 << 63)
    return m


def wide_order(a, key):
    """the stable order of 16-byte keys: by the mapped high limb, then the low one"""
    m = wide_mapped(a, key)
    return np.lexsort((m[:, 0], m[:, 1]))


def wide_sorted(a, key):
    return a[wide_order(a, key)]


def wide_digits(m, level):
    """the digit of every row of (mapped) limbs at `level`, 0 (the lowest byte of `low`) to 15"""
    return ((m[:, level // 8] >> np.uint64(8 * (level % 8))) & np.uint64(0xFF)).astype(np.int64)


def wide_with_constant_levels(n, key, levels, seed, digit=0x5A):
    """the limb form of keys_with_constant_levels: random 16-byte keys whose MAPPED bytes at `levels` all hold `digit`"""
    m = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 2), dtype=np.uint64, endpoint=False)
    for l in levels:
        sh = np.uint64(8 * (l % 8))
        m[:, l // 8] = (m[:, l // 8] & ~(np.uint64(0xFF) << sh)) | (np.uint64(digit) << sh)
    return wide_mapped(m, key)


def wide_constant_levels(a, key):
    """the limb form of constant_levels"""
    m = wide_mapped(a, key)
    return {l for l in range(16) if (wide_digits(m, l) == wide_digits(m[:1], l)[0]).all()}


def wide_heavy_digit_inputs(n, key, level, seed, run=1000):
    """the limb form of heavy_digit_inputs: its digit shapes at `level` of the MAPPED key, every other byte random"""
    other = np.random.default_rng([seed, 16]).integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)
    out = {}
    for name, limb in heavy_digit_inputs(n, "uint64", level % 8, seed, run).items():
        m = np.empty((n, 2), dtype=np.uint64)
        m[:, level // 8], m[:, 1 - level // 8] = limb, other
        out[name] = wide_mapped(m, key)
    return out


# ---- the wide [u8; N] route's refinement rounds: rows with a known order, and §2d's loop restated --------------------------
# The library's constants, quoted from rdst_amd/csrc/rdst_bytes.hip (tests/test_bytes_rounds_inputs.py reads the constexpr
# lines and compares):
BYTES_SMALL = 256                # longest run the comparison kernel takes
CMP_WORDS = 3840                 # its staging budget per wave, in u32 words
CMP_WAVES = 4                    # runs per workgroup of short_runs_kernel
BYTES_GRID_CAP = 256 * 16        # GRID_CAP: workgroups (of 256 threads) of the grid-stride kernels
BYTES_SCAN_TILE = 256 * 16       # SCAN_TILE: items per tile of the scans
SHORT_RUNS_BLOCKS = 1 << 20      # bytes_order: `if (blocks > (1u << 20)) blocks = 1u << 20;`
GRID_ROWS = BYTES_GRID_CAP * 256             # rows one trip of a grid-stride kernel covers
SHORT_RUNS_PER_TRIP = SHORT_RUNS_BLOCKS * CMP_WAVES

ROUND_KINDS = ("word0", "later", "last", "straddle", "dup")   # where a run's deciding bytes fall; "+dups": a third repeats
ROUND_ID_BITS = 16               # ids stay below 2^16: the int64 (run, id) key is run << 16 | id


def run_is_long(length, words):
    """run_is_long of rdst_bytes.hip: too many rows for four per lane, or too many words to stage"""
    return length > BYTES_SMALL or length * words > CMP_WORDS


def long_round_bits(long_runs):
    """(b, k) of a long round: b = ceil(log2(long runs)) bits of run ordinal, k = (64 - b) / 8 whole key bytes"""
    b = 0 if long_runs <= 1 else (long_runs - 1).bit_length()
    return b, (64 - b) // 8


def _trips(items, per_trip):
    return -(-items // per_trip)


def bytes_first_round(lengths, N):
    """The first refinement round of rows whose 8-byte prefixes differ from run to run, from the runs' lengths alone (what
    bytes_round_census reports as its round 0): the form the full-size device cases are held to."""
    lengths = np.asarray(lengths, dtype=np.int64)
    words = (N - 8 + 3) // 4
    tied = lengths[lengths >= 2]
    is_long = (tied > BYTES_SMALL) | (tied * words > CMP_WORDS)
    long, short = tied[is_long], tied[~is_long]
    b, k = long_round_bits(len(long))
    m = int(lengths.sum())
    return dict(depth=8, words=words, m=m, tied=int(tied.sum()), runs=len(tied), long_rows=int(long.sum()), long_runs=len(long),
                b=b, k=k, short_max=int(short.max()) if len(short) else 0, scan_trips=_trips(m, GRID_ROWS),
                short_trips=_trips(len(short), SHORT_RUNS_PER_TRIP), long_trips=_trips(int(long.sum()), GRID_ROWS))


def bytes_round_census(rows_sorted, N):
    """DESIGN.md §2d's loop restated in numpy over the SORTED rows (n, N): one dict per refinement round with what the host
    reads (tied rows, runs, long rows, long runs), the round's depth, words, b and k, the longest short run, and the trips the
    grid-stride loops make: `scan_trips` long_rows_kernel over the round's m rows, `short_trips` short_runs_kernel over its
    runs (0: not launched), `long_trips` bytes_keys_kernel and both slot kernels over the long rows."""
    rows = np.asarray(rows_sorted)
    n = rows.shape[0]
    assert rows.shape == (n, N) and rows.dtype == np.uint8 and N > 8
    # group[i]: the rows i - 1 and i are still tied; active: the rows the round looks at (positions in sorted order)
    same = np.ones(n, dtype=bool)
    same[1:] = (rows[1:, :8] == rows[:-1, :8]).all(axis=1)
    same[0] = False
    active = np.arange(n)
    depth, out = 8, []
    while depth < N:
        words = (N - depth + 3) // 4
        m = len(active)
        heads = np.flatnonzero(~same[active]) if m else np.arange(0)      # run heads among the active rows
        lens = np.diff(np.append(heads, m))
        tied_mask = lens >= 2
        tlen, thead = lens[tied_mask], heads[tied_mask]
        long_mask = (tlen > BYTES_SMALL) | (tlen * words > CMP_WORDS)
        long_runs, long_rows = int(long_mask.sum()), int(tlen[long_mask].sum())
        b, k = long_round_bits(long_runs)
        short = tlen[~long_mask]
        out.append(dict(depth=depth, words=words, m=m, tied=int(tlen.sum()), runs=len(tlen), long_rows=long_rows, long_runs=long_runs,
                        b=b, k=k, short_max=int(short.max()) if len(short) else 0, scan_trips=_trips(m, GRID_ROWS),
                        short_trips=_trips(len(short), SHORT_RUNS_PER_TRIP), long_trips=_trips(long_rows, GRID_ROWS)))
        if len(tlen) == 0 or long_runs == 0:
            break
        keep = np.concatenate([np.arange(h, h + l) for h, l in zip(thead[long_mask], tlen[long_mask])])
        nxt = active[keep]
        first = np.zeros(len(nxt), dtype=bool)
        first[np.cumsum(tlen[long_mask])[:-1]] = True
        first[0] = True
        chunk = rows[nxt, depth:min(depth + k, N)]                         # (bytes past N are zero for every row)
        differs = np.ones(len(nxt), dtype=bool)
        differs[1:] = (chunk[1:] != chunk[:-1]).any(axis=1)
        same = same.copy()
        same[nxt] = ~(first | differs)
        active, depth = nxt, depth + k
    return out


def spread_runs(runs, singles):
    """`runs` spread evenly among `singles` unrelated rows (runs of one row): the list bytes_round_rows takes"""
    out, gap = [], singles // (len(runs) + 1)
    for r in runs:
        out += [(1, "word0")] * gap + [r]
    return out + [(1, "word0")] * (singles - gap * len(runs))


def _mix(x):
    """a byte from an int64 (wrapping multiply, a middle byte of the product)"""
    return ((x * 0x2545F4914F6CDD1D) >> 29) & 0xFF


def bytes_round_rows(torch, lengths, kinds, N, k=8, seed=0, device="cpu", dups=None):
    """Rows of [u8; N], N > 8, whose sorted order is known without sorting.  Run r (lengths[r] rows) has the big-endian prefix
    r * scale + (an offset below scale): strictly increasing.  The N - 8 bytes behind it come from a per-row integer id, in
    the field its kind names, big-endian — before the field every byte is the run's own, behind it a function of (run, id) —
    so id order is the lexicographic order and equal ids are equal rows:
      word0      ids in suffix bytes [0, 2): decided in the comparison kernel's first word
      later      ids in the first two bytes of suffix word 1 + run % (whole words - 1): word 0 never decides
      last       ids in the last byte alone (0x00 and 0x01 among them); more than 256 rows repeat
      straddle   id = hi << 8 | lo, hi at row byte 8 + k - 1, lo at 8 + k, sixteen rows to a hi: the round that takes k bytes
                 leaves them tied in sixteens, the next byte separates them
      dup        every row the same
    `kinds`: indices into ROUND_KINDS; `dups`: runs in which every third row repeats the row before it.  `lengths`, `kinds`,
    `dups`: sequences or tensors, one entry per run.  Returns a dict: `sorted` (n, N) uint8, `rows` = sorted[perm] with a
    seeded `perm`, `key` (the int64 run << 16 | id of the sorted rows) and `key_shuffled` = key[perm]."""
    i64 = torch.int64
    lengths = torch.as_tensor(lengths, dtype=i64, device=device)
    kinds = torch.as_tensor(kinds, dtype=i64, device=device)
    dups = torch.zeros_like(lengths, dtype=torch.bool) if dups is None else torch.as_tensor(dups, dtype=torch.bool, device=device)
    R, S = lengths.numel(), N - 8
    assert N > 8 and 1 <= k <= 8 and int(lengths.min()) >= 1 and int(lengths.max()) <= 4096
    n = int(lengths.sum())
    run = torch.repeat_interleave(torch.arange(R, device=device, dtype=i64), lengths)
    start = torch.cumsum(lengths, 0) - lengths
    i = torch.arange(n, device=device, dtype=i64) - start[run]
    ln, kd = lengths[run], kinds[run]
    j = i - (dups[run] & (i % 3 == 2)).to(i64)
    W0, LATER, LAST, STRADDLE, DUP = range(5)
    if bool((kinds == LATER).any()):
        assert S >= 6, "no word behind word 0 to decide in"
    if bool((kinds == STRADDLE).any()):
        assert k + 1 <= S, "the straddled byte pair lies past N"
    width = torch.where(kd == LAST, 1, 2)
    cap = torch.where(kd == LAST, 256, 65536)
    stride = torch.clamp((cap - 1) // torch.clamp(ln - 1, min=1), min=1)
    ident = torch.where(ln <= cap, torch.where(j == 1, 1, j * stride), j * cap // ln)
    ident = torch.where(kd == STRADDLE, (j // 16) * 256 + (j % 16) * 17, ident)
    ident = torch.where(kd == DUP, 0, ident)
    assert int(ident.max()) < (1 << ROUND_ID_BITS)
    later_words = max(1, (S - 2) // 4)                       # the words 1 .. later_words hold two whole bytes
    f0 = torch.where(kd == W0, 0, torch.where(kd == LATER, 4 * (1 + run % later_words), torch.where(kd == LAST, S - 1, k - 1)))
    f0 = torch.where(kd == DUP, S, f0)
    width = torch.where(kd == DUP, 0, width)
    # the prefix
    scale = ((1 << 63) - 1) // R
    v = run * scale + ((run * 2654435761) & 0x7FFFFFFF) % scale
    shifts = torch.arange(56, -8, -8, device=device, dtype=i64)
    prefix = (v[:, None] >> shifts[None, :]) & 0xFF
    # the suffix
    P = torch.arange(S, device=device, dtype=i64)[None, :]
    f0c, wc = f0[:, None], width[:, None]
    own = _mix(run[:, None] * 0x9E3779B1 + P * 0x85EBCA6B + 1)
    behind = _mix(run[:, None] * 0x9E3779B1 + P * 0x85EBCA6B + (ident[:, None] + 1) * 0xC2B2AE35)
    field = (ident[:, None] >> (8 * torch.clamp(f0c + wc - 1 - P, min=0, max=7))) & 0xFF
    suffix = torch.where(P < f0c, own, torch.where(P < f0c + wc, field, behind))
    rows = torch.cat([prefix, suffix], dim=1).to(torch.uint8)
    key = (run << ROUND_ID_BITS) | ident
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    perm = torch.randperm(n, generator=gen, device=device)
    return {"sorted": rows, "rows": rows[perm], "perm": perm, "key": key, "key_shuffled": key[perm], "N": N, "n": n}


def bytes_round_case(torch, runs, N, k=8, seed=0, device="cpu"):
    """bytes_round_rows for a list of runs (length, kind), kind a name of ROUND_KINDS, "+dups" appended for a run in which a
    third of the rows repeat"""
    lengths = [r[0] for r in runs]
    kinds = [ROUND_KINDS.index(r[1].split("+")[0]) for r in runs]
    dups = [r[1].endswith("+dups") for r in runs]
    return bytes_round_rows(torch, lengths, kinds, N, k, seed, device, dups)


RECORD_JUNK = 3                  # random bytes directly behind the key: a read past N changes the order


def bytes_round_records(case, seed):
    """The records form of a (host) case: rows `tag(u1) | key(N) | junk(3) | seq(<u4)`, R = N + 8, the key at the odd offset
    1, random junk directly behind it, seq = arange(n) in shuffled (input) order, tag one of three values.  Returns the raw
    (n, R) uint8 input, its structured view's dtype, and the two expected outputs: `by_key` — the stable order on the int64
    (run, id) key — and `by_key_tag_desc` — the stable order on (key ascending, tag descending)."""
    N, n = case["N"], case["n"]
    rng = np.random.default_rng(seed)
    dt = np.dtype({"names": ["tag", "k", "junk", "seq"], "formats": ["u1", ("u1", (N,)), ("u1", (RECORD_JUNK,)), "<u4"],
                   "offsets": [0, 1, 1 + N, 1 + N + RECORD_JUNK], "itemsize": N + 8})
    raw = np.zeros((n, dt.itemsize), dtype=np.uint8)
    raw[:, 0] = rng.integers(0, 3, size=n, dtype=np.uint8)
    raw[:, 1:1 + N] = case["rows"].cpu().numpy()
    raw[:, 1 + N:1 + N + RECORD_JUNK] = rng.integers(0, 256, size=(n, RECORD_JUNK), dtype=np.uint8)
    raw[:, 1 + N + RECORD_JUNK:] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)
    key = case["key_shuffled"].cpu().numpy()
    by_key = raw[np.argsort(key, kind="stable")]
    by_key_tag = raw[np.argsort(key * 4 + (3 - raw[:, 0].astype(np.int64)), kind="stable")]
    return {"raw": raw, "dtype": dt, "by_key": by_key, "by_key_tag_desc": by_key_tag}


# The cases of tests/test_gpu_bytes_rounds.py, as (name, runs, N, k): built here so that the CPU test of the inputs and the
# GPU test use the same lists.
RANK_WIDTHS = (20, 41, 68)       # 3 words; 9 words, the last one byte and three of padding; 15 words
RANK_LENGTHS = (2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
RANK_KINDS = ("later", "last+dups", "straddle", "word0+dups", "dup", "later+dups", "last", "straddle+dups", "word0")
BUDGET_PAIRS = ((68, 256, 257), (72, 240, 241), (1000, 15, 16), (3848, 4, 5), (3849, 3, 4), (4096, 3, 4))   # N, short, long
LAYOUT_LONG_RUNS = {1: (0, 8), 2: (1, 7), 3: (2, 7), 256: (8, 7), 257: (9, 6), 65536: (16, 6), 65537: (17, 5)}   # -> (b, k)
LAYOUT_KINDS = ("straddle", "last", "straddle+dups", "last+dups", "dup", "word0")
STRIDE_PAIRS, STRIDE_MID = 4_200_000, 2_000     # the runs of the short-run grid-stride case


def ranking_runs(N):
    """three runs of every length of RANK_LENGTHS, the kinds dealt round (9 kinds, 39 runs: every length meets three kinds,
    every kind at least four lengths), among 5 000 unrelated rows; the straddled pair is suffix bytes 3 and 4: the border
    of the comparison kernel's words 0 and 1"""
    runs = [(length, RANK_KINDS[(3 * a + rep) % len(RANK_KINDS)]) for a, length in enumerate(RANK_LENGTHS) for rep in range(3)]
    return spread_runs(runs, 5000), 4


def budget_runs(N, short, long):
    """one run on each side of len * words = CMP_WORDS, distinct rows decided in the last byte, among 40 unrelated rows"""
    return spread_runs([(short, "last"), (long, "last")], 40), 8


def layout_runs(long_runs, scale=1):
    """`long_runs` runs of 257 rows (the shortest long run), the kinds of LAYOUT_KINDS dealt round, a few short runs and
    unrelated rows between them; k is the first long round's"""
    k = long_round_bits(long_runs)[1]
    runs = [(BYTES_SMALL + 1, LAYOUT_KINDS[r % len(LAYOUT_KINDS)]) for r in range(long_runs)]
    extra = [(2, "last"), (64, "straddle"), (200, "later+dups"), (256, "last")]
    step = max(1, long_runs // 4)
    out = []
    for r, item in enumerate(runs):
        if r % step == 0 and r // step < len(extra):
            out += [(1, "word0")] * 5 + [extra[r // step]]
        out.append(item)
    return out + [(1, "word0")] * 5, k


def layout_tensors(torch, long_runs, device):
    """layout_runs(long_runs) without the extras, as tensors: every run 257 rows, kinds and "+dups" as LAYOUT_KINDS deals
    them (the two largest cases are built on the device)"""
    r = torch.arange(long_runs, device=device, dtype=torch.int64)
    names = [ROUND_KINDS.index(kname.split("+")[0]) for kname in LAYOUT_KINDS]
    kinds = torch.tensor(names, device=device, dtype=torch.int64)[r % len(LAYOUT_KINDS)]
    dups = torch.tensor([kname.endswith("+dups") for kname in LAYOUT_KINDS], device=device)[r % len(LAYOUT_KINDS)]
    return torch.full_like(r, BYTES_SMALL + 1), kinds, dups


def stride_tensors(torch, device, pairs=STRIDE_PAIRS, mid=STRIDE_MID):
    """`pairs` runs of 2 rows with `mid` runs of 65 ... 256 rows spread evenly through them, all decided in the last byte
    (alternately with a third of the rows repeating)"""
    total = pairs + mid
    r = torch.arange(total, device=device, dtype=torch.int64)
    every = total // mid
    is_mid = (r % every == every // 2) & (r // every < mid)
    lengths = torch.where(is_mid, 65 + (r // every) * 37 % 192, 2)
    kinds = torch.full_like(r, ROUND_KINDS.index("last"))
    dups = is_mid & ((r // every) % 2 == 1)
    return lengths, kinds, dups
