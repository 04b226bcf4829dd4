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
