"""Where the sorts read and write.  Every entry point and route runs on views inside a larger allocation, at addresses of
every residue the kernels' vector forms care about, with guard bands of known bytes on both sides (tests/helpers.py,
Bands): seeded random bytes, which catch stray writes, and the bit pattern of the type's smallest mapped key, with every
occurrence of that key taken out of the input, which catches band elements read as keys.  Each case checks three things:
the result against the reference order, every band byte for byte, and the device error word.  Read-only inputs and slices
of length 0 and 1 must stay untouched inside as well."""
import ctypes

import numpy as np
import pytest

from helpers import (BAND_BYTES, Bands, giant_buckets_input, heavy_digit_inputs, mapped_key, poison_pattern, random_bits,
                     reference_sorted, same_bits, to_host, with_prefixes, without_poison)

pytestmark = pytest.mark.gpu

SMALL_LIMIT = {1: 16384, 2: 16384, 4: 16384, 8: 8192, 16: 4096}   # the one-workgroup sort: 1 024 threads x keys per thread
K3_TILE = 21_504                                                   # the largest scatter tile (keys)
R1 = "0x100"    # the round-1 geometry: the view starts 0x100 after the end of a banded neighbour
PLACEMENTS = {  # (keys, tmp) byte offsets: residues modulo 16, element-aligned
    1: ((1, 2), (3, 1)),
    2: ((2, 6), (6, 0)),
    4: ((0, 0), (0, 4), (4, 0), (8, 12), (12, 12)),
    8: ((0, 0), (0, 8), (8, 0), (8, 8)),
    16: ((0, 0), (16, 48)),
}
MIXED = {1: (3, 1), 2: (2, 6), 4: (8, 12), 8: (0, 8), 16: (16, 48)}   # one placement with keys and tmp on different residues
RUNS = (("random", "random"), ("random", "poison"), ("sorted", "poison"), ("equal", "random"))
RUNS_BIG = (("random", "poison"), ("sorted", "random"), ("equal", "poison"))   # from a million keys up: each fill still seen


@pytest.fixture
def route(gpu):
    yield gpu
    gpu.set_hybrid(True, 0)
    gpu.device_status()


def _nbytes(key):
    return 16 if key == "u128" else np.dtype(key).itemsize


def _dtype(key):
    return "uint64" if key == "u128" else key


def _ref(a, key=None):
    if key == "u128":
        return a[np.lexsort((a[:, 0], a[:, 1]))]
    return reference_sorted(a)


def _random(n, key, seed):
    if key == "u128":
        return random_bits(2 * n, "uint64", seed).reshape(n, 2).copy()
    return random_bits(n, key, seed).copy()


def _input(kind, a, key=None):
    if kind == "sorted":
        return _ref(a, key)
    if kind == "equal":
        return np.repeat(a[:1], a.shape[0], axis=0)
    return a


def _fill(fill, key):
    return poison_pattern(key) if fill == "poison" else "random"


def _place(name, init, offset, fill, seed, device="cuda"):
    """(Bands holding `name` at `offset`, names of the views besides it that must stay untouched)"""
    if offset == R1:
        neighbour = random_bits(16384, "uint32", seed + 1)      # 64 KiB: its end is 256-aligned
        return Bands([("neighbour", neighbour, 0), (name, init, 0x100)], seed=seed, fill=fill, device=device), ("neighbour",)
    return Bands([(name, init, offset)], seed=seed, fill=fill, device=device), ()


def _placements(nb):
    return PLACEMENTS[nb] + ((R1, R1),)


def _sort_abi(keys, tmp, n, key):
    """rdst_hip_sort_device itself (the Python wrapper returns before the library for n <= 1)"""
    import torch
    from rdst_amd import _lib
    from rdst_amd.radix_sort import key_info
    kind, nbytes, levels = key_info(key)
    _lib.check(_lib.load().rdst_hip_sort_device(ctypes.c_void_p(keys.data_ptr()), ctypes.c_void_p(tmp.data_ptr()), n, nbytes, kind,
                                               levels, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _case(kind, fill, a, key=None):
    """(input, expected result) of one run: the input without the poison key when the bands hold it"""
    x = _input(kind, a, key)
    if fill == "poison":
        x = without_poison(x, key)
    return x, _ref(x, key)


def _runs(n):
    return RUNS if n < 1_000_000 else RUNS_BIG


def _banded_sort(gpu, a, exp, key, placement, fill, seed, tmp_extra=0, what=""):
    """sort `a` in place in a banded view with a banded tmp; asserts the result (`exp`), the bands and the error word;
    returns the route the library reports"""
    pat = _fill(fill, key)
    koff, toff = placement
    kb, kt = _place("keys", a, koff, pat, seed)
    tb, tt = _place("tmp", (a.shape, a.dtype), toff, pat, seed + 7)
    n = a.shape[0]
    tmp = tb.extended("tmp", tmp_extra) if tmp_extra else tb["tmp"]
    if n <= 1:
        _sort_abi(kb["keys"], tmp, n, key)
    else:
        gpu.sort_device_tensor(kb["keys"], tmp, check=False, key=key if key == "u128" else None)
    gpu.device_status()
    route = gpu.last_route()
    what = f"{what} {key} n={n} placement={placement} fill={fill}"
    assert same_bits(to_host(kb["keys"], _dtype(key)), exp), what
    kb.check(what, untouched=kt + (("keys",) if n <= 1 else ()))
    tb.check(what, untouched=tt + (("tmp",) if n <= 1 else ()))
    return route


def _rows(gpu, key, n, placements, seed, tmp_extra=0, want=None, what="", base=None):
    """RUNS at every placement at one length; `want`: the route random input must report"""
    a = _random(n, key, seed) if base is None else base
    cases = {(kind, fill): _case(kind, fill, a, key) for kind, fill in _runs(n)}
    for p in placements:
        for (kind, fill), (x, exp) in cases.items():
            got = _banded_sort(gpu, x, exp, key, p, fill, seed, tmp_extra, f"{what} {kind}")
            if want and kind == "random":
                assert got == want, (what, key, n, p, fill, got)


# ---- sort_device_tensor: the one-workgroup sort, LSD, hybrid, giant buckets, atomic, split -------------------------

@pytest.mark.parametrize("key", ("uint8", "int8", "uint16", "int16", "uint32", "int32", "float32", "uint64", "int64", "float64",
                                 "u128"))
def test_one_workgroup_sort_stays_in_its_slice(route, key):
    nb = _nbytes(key)
    lim = SMALL_LIMIT[nb]
    for n in (0, 1, 2, 3, 63, 64, 65, lim - 1, lim, lim + 1):
        _rows(route, key, n, _placements(nb), seed=n + nb, what="default")


@pytest.mark.parametrize("key", ("uint32", "float32", "int64", "float64", "uint16", "int8", "u128"))
def test_lsd_route_stays_in_keys_and_tmp(route, key):
    """tmp is handed over with half a band more than len elements: what lies past len must stay as it was"""
    route.set_hybrid(False)
    nb = _nbytes(key)
    for n in (K3_TILE - 1, K3_TILE + 1, 8 * K3_TILE + 31, 1_000_003):
        places = _placements(nb) if n < 1_000_000 else (MIXED[nb], (R1, R1))
        _rows(route, key, n, places, seed=n, tmp_extra=BAND_BYTES // 2, want="lsd", what="lsd")


@pytest.mark.parametrize("key,mode", (("uint32", 7), ("float32", 7), ("int64", 7), ("float64", 7), ("uint64", 6), ("int64", 15)))
def test_hybrid_route_stays_in_keys_and_tmp(route, key, mode):
    """the K1h hybrid route (mode 7; 8-byte keys also with the one-block-per-CU K4, mode 6) and the second form of the 8-byte
    K4 behind the atomic route (mode 15)"""
    route.set_hybrid(mode, 1)
    nb = _nbytes(key)
    want = "atomic" if mode == 15 else "hybrid"
    for n in (300_001, 3_000_001):
        places = _placements(nb) if n < 1_000_000 else (MIXED[nb], (R1, R1))
        _rows(route, key, n, places, seed=n + mode, want=want, what=f"mode {mode}")
    # ~200 buckets of ~9 000 keys: most of a K4 tile, next to the bands
    a = with_prefixes(200 * 9000, key, list(range(7, 207)), seed=400)
    for kind, fill in (("random", "poison"), ("sorted", "random")):
        _banded_sort(route, *_case(kind, fill, a), key, MIXED[nb], fill, 401, what=f"mode {mode} prefixes {kind}")


@pytest.mark.parametrize("key", ("uint32", "int32", "float32"))
def test_hybrid_giant_buckets_next_to_the_bands(route, key):
    """the input of test_giant_buckets: buckets of 65 536 keys and more, at the first and the last prefix among them"""
    route.set_hybrid(7, 1)
    a = giant_buckets_input(np.random.default_rng(2024), key)
    _rows(route, key, a.shape[0], ((4, 0), (12, 12), (R1, R1)), seed=2024, want="hybrid", what="giants", base=a)


@pytest.mark.parametrize("key", ("uint32", "float32", "uint64", "float64"))
def test_atomic_route_stays_in_keys_and_tmp(route, key):
    route.set_hybrid(True, 1)
    nb = _nbytes(key)
    _rows(route, key, 1_000_003, _placements(nb), seed=1, want="atomic", what="atomic")
    _rows(route, key, 5_000_011, (MIXED[nb],), seed=5, want="atomic", what="atomic")


def test_atomic_route_at_two_pow_25_keys(route):
    """a length at which the atomic route's areas take several tiles each"""
    route.set_hybrid(True, 1)
    n = (1 << 25) + 1_021
    a = random_bits(n, "uint32", 0x5D570B25).copy()
    s = np.sort(a)
    for kind, fill in (("random", "random"), ("sorted", "poison")):
        b = {"random": a, "sorted": s}[kind]
        if fill == "poison":
            b = without_poison(b)
        kb, _ = _place("keys", b, 8, _fill(fill, "uint32"), 1)
        tb, _ = _place("tmp", (n, "uint32"), 12, _fill(fill, "uint32"), 2)
        route.sort_device_tensor(kb["keys"], tb["tmp"])
        r = route.last_route()
        assert kind != "random" or r == "atomic", r
        assert np.array_equal(to_host(kb["keys"], "uint32"), np.sort(b)), kind
        kb.check(kind)
        tb.check(kind)
        del kb, tb


@pytest.mark.parametrize("key", ("uint32", "float32", "int64", "float64"))
def test_split_parts_stay_in_keys_and_tmp(route, key):
    """the split forced at every length (eight parts at arbitrary offsets into keys and tmp); the parts of a slice below
    2^26 keys end on the hybrid route"""
    route.set_hybrid(17, 1)
    nb = _nbytes(key)
    places = {4: ((0, 4), (4, 0), (8, 12)), 8: ((0, 8), (8, 0))}[nb] + ((R1, R1),)
    _rows(route, key, 100_003, places, seed=0x5D570B17)
    _rows(route, key, 3_000_001, (MIXED[nb], (R1, R1)), seed=0x5D570B18, want="hybrid", what="split")


# ---- key-value sorts ---------------------------------------------------------------------------------------------

PAIR_PLACES = {  # (keys, vals, tmp_keys, tmp_vals)
    (4, 4): ((0, 4, 8, 12), (12, 8, 4, 0)), (4, 8): ((4, 8, 12, 0), (8, 0, 0, 8)),
    (8, 4): ((8, 4, 0, 12), (0, 12, 8, 4)), (8, 8): ((0, 8, 8, 0), (8, 0, 0, 8)),
}


@pytest.mark.parametrize("key,val", (("uint32", "uint32"), ("uint32", "uint64"), ("float32", "int64"), ("uint64", "uint32"),
                                     ("float64", "uint64")))
def test_pairs_stay_in_keys_values_and_both_tmps(gpu, key, val):
    nk, nv = np.dtype(key).itemsize, np.dtype(val).itemsize
    for n in (K3_TILE - 1, K3_TILE + 1, 2_000_003):
        a = _random(n, key, n)
        v = np.arange(n, dtype=val)
        places = PAIR_PLACES[(nk, nv)] if n < 1_000_000 else PAIR_PLACES[(nk, nv)][:1]
        for p in places + ((R1, R1, R1, R1),):
            for kind, fill in _runs(n):
                k = _case(kind, fill, a)[0]
                bands = [_place("keys", k, p[0], _fill(fill, key), 1), _place("vals", v, p[1], _fill(fill, val), 2),
                         _place("tmp_keys", (n, key), p[2], _fill(fill, key), 3), _place("tmp_vals", (n, val), p[3], _fill(fill, val), 4)]
                (kb, _), (vb, _), (tkb, _), (tvb, _) = bands
                gpu.sort_pairs_device_tensor(kb["keys"], vb["vals"], tkb["tmp_keys"], tvb["tmp_vals"])
                perm = np.argsort(mapped_key(k), kind="stable")
                what = f"pairs {key}/{val} n={n} placement={p} {kind} fill={fill}"
                assert same_bits(to_host(kb["keys"], key), k[perm]), what
                assert np.array_equal(to_host(vb["vals"], val), v[perm]), what
                for b, untouched in bands:
                    b.check(what, untouched=untouched)


# ---- the low-memory route and partition_device -------------------------------------------------------------------

SCRATCH = 65_536 + 1_000   # not a multiple of 4 096: the route uses only the rounded-down part; the band starts at numel


@pytest.mark.parametrize("key,off", (("uint32", 4), ("float32", 12), ("int64", 8)))
def test_lowmem_and_partition_stay_in_keys_and_scratch(gpu, key, off):
    """keys at a residue that is not 16-byte aligned: every tile the route copies starts unaligned"""
    levels = np.dtype(key).itemsize
    w = 8 * levels
    for n in (1_000_003, 3_000_001):
        a = _random(n, key, n)
        for kind, fill in RUNS if n < 2_000_000 else RUNS_BIG:
            k, exp = _case(kind, fill, a)
            what = f"lowmem {key} n={n} {kind} fill={fill}"
            kb, _ = _place("keys", k, off, _fill(fill, key), 1)
            sb, _ = _place("scratch", (SCRATCH, key), 0, _fill(fill, key), 2)
            gpu.sort_device_tensor_lowmem(kb["keys"], sb["scratch"])
            gpu.device_status()
            assert same_bits(to_host(kb["keys"], key), exp), what
            kb.check(what)
            sb.check(what)
            # partition_index on the top digit of the first key (as tests/test_gpu_lowmem.py: split index, both sides)
            level, digit = levels - 1, int(mapped_key(k[:1])[0] >> np.array(w - 8, dtype=f"uint{w}"))
            kb, _ = _place("keys", k, off, _fill(fill, key), 3)
            sb, _ = _place("scratch", (SCRATCH, key), 0, _fill(fill, key), 4)
            split = gpu.partition_device(kb["keys"], level, digit, sb["scratch"])
            got = to_host(kb["keys"], key)
            dg = (mapped_key(got) >> np.array(w - 8, dtype=f"uint{w}")).astype(np.int64)
            want = int(((mapped_key(k) >> np.array(w - 8, dtype=f"uint{w}")).astype(np.int64) == digit).sum())
            assert split == want and (dg[:split] == digit).all() and (dg[split:] != digit).all(), what
            assert same_bits(reference_sorted(got), exp), what
            kb.check("partition " + what)
            sb.check("partition " + what)


# ---- [u8; N] rows --------------------------------------------------------------------------------------------------

ROW_OFFSETS = (0, 1, 3, 4, 8)   # with the strides below: every gather unit (16, 8, 4, 1 bytes) is taken at least once


def _byte_rows(rng, n, N):
    a = rng.integers(0, 256, size=(n, N), dtype=np.uint8)
    a[rng.random((n, N)) < 0.3] = 0
    return a


def _rows_sorted(a):
    n, N = a.shape
    return a.copy() if n == 0 else np.sort(a.view(f"V{N}").ravel()).view(np.uint8).reshape(n, N)


@pytest.mark.parametrize("N", (1, 3, 4, 5, 8, 12, 16, 17, 24, 33, 100, 4096))
def test_bytes_rows_stay_in_rows_and_scratch(gpu, N):
    """rows at byte offsets {0, 1, 3, 4, 8}; a scratch of exactly rdst_hip_sort_bytes_scratch_bytes at a 256-aligned start,
    the band right behind it"""
    import torch
    from rdst_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(0xB0 + N)
    for n in (0, 1, 2, 257, 100_003 if N < 4096 else 2_000):
        a = _byte_rows(rng, n, N)
        need = int(lib.rdst_hip_sort_bytes_scratch_bytes(n, N)) if n > 1 else 0
        for off in ROW_OFFSETS:
            runs = RUNS if off in (0, 1) else (("random", "random"),)
            for kind, fill in runs:
                r = {"random": a, "sorted": _rows_sorted(a), "equal": np.repeat(a[:1], n, axis=0)}[kind]
                if fill == "poison":
                    r = without_poison(r, "bytes")
                what = f"[u8; {N}] n={n} offset={off} {kind} fill={fill}"
                rb, _ = _place("rows", r, off, _fill(fill, "bytes"), 1)
                sb, _ = _place("scratch", (need, "uint8"), 0, _fill(fill, "bytes"), 2)
                if n > 1:
                    gpu.sort_bytes_device_tensor(rb["rows"], sb["scratch"], check=False)
                else:
                    _lib.check(lib.rdst_hip_sort_bytes_device(ctypes.c_void_p(rb["rows"].data_ptr()), n, N,
                                                              ctypes.c_void_p(sb["scratch"].data_ptr()), need,
                                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
                gpu.device_status()
                assert np.array_equal(rb["rows"].cpu().numpy(), _rows_sorted(r)), what
                rb.check(what, untouched=("rows",) if n <= 1 else ())
                sb.check(what)


# ---- the parity hooks and the sharded sort's local steps -----------------------------------------------------------

def _digits(a, level):
    m = mapped_key(a)
    return ((m >> np.array(8 * level, dtype=m.dtype)) & np.array(0xFF, dtype=m.dtype)).astype(np.int64)


@pytest.mark.parametrize("key", ("uint32", "int64", "float32"))
def test_hooks_read_only_their_source_and_write_only_dst(gpu, key):
    """scatter_level, level_counts, all_level_counts: the source stays untouched inside and out, dst is banded"""
    levels = np.dtype(key).itemsize
    for n in (9, 250_000):
        a = _random(n, key, n)
        inputs = {"random": a, "sorted": reference_sorted(a), "90% one digit": heavy_digit_inputs(n, key, 0, n)["90% one digit"]}
        for (name, src), off in zip(inputs.items(), (levels, 0, R1)):
            what = f"hooks {key} n={n} {name} src offset {off}"
            sb, st = _place("src", src, off, "random", 1)
            for level in (0, levels - 1):
                db, _ = _place("dst", (n, key), levels if off == 0 else 0, "random", 2)
                _dst, counts = gpu.scatter_level(sb["src"], level, db["dst"])
                gpu.device_status()
                d = _digits(src, level)
                assert same_bits(to_host(db["dst"], key), src[np.argsort(d, kind="stable")]), (what, level)
                assert np.array_equal(counts.astype(np.int64), np.bincount(d, minlength=256)), (what, level)
                db.check(f"{what} level {level}")
                c, _srt, _first, _last = gpu.level_counts(sb["src"], level)
                assert np.array_equal(np.asarray(c, dtype=np.int64), np.bincount(d, minlength=256)), (what, level)
            allc = gpu.all_level_counts(sb["src"])
            for level in range(levels):
                assert np.array_equal(allc[level].astype(np.int64), np.bincount(_digits(src, level), minlength=256)), (what, level)
            sb.check(what, untouched=("src",) + st)


@pytest.mark.parametrize("key", ("uint32", "float64"))
def test_split_steps_stay_in_their_buffers(gpu, key):
    """rdst_hip_split_top_level_device (src read-only) and rdst_hip_split_top16_device, through the C ABI: every buffer and
    both count arrays (256 and 65 536 x u64) banded"""
    import torch
    from rdst_amd import _lib
    from rdst_amd.radix_sort import key_info
    lib = _lib.load()
    kind_code, nbytes, _levels = key_info(key)
    w = 8 * nbytes
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = 1_000_003
    a = _random(n, key, 0x5D570B30)
    for kind in ("random", "sorted", "equal"):
        src = _input(kind, a)
        m = mapped_key(src)
        top8 = (m >> np.array(w - 8, dtype=m.dtype)).astype(np.int64)
        top16 = (m >> np.array(w - 16, dtype=m.dtype)).astype(np.int64)
        what = f"split steps {key} {kind}"
        sb, st = _place("src", src, 8, "random", 1)
        db, _ = _place("dst", (n, key), 0, "random", 2)
        cb, _ = _place("counts", (256, "uint64"), 8, "random", 3)
        _lib.check(lib.rdst_hip_split_top_level_device(ctypes.c_void_p(sb["src"].data_ptr()), ctypes.c_void_p(db["dst"].data_ptr()),
                                                       n, nbytes, kind_code, ctypes.c_void_p(cb["counts"].data_ptr()), stream))
        gpu.device_status()
        assert same_bits(to_host(db["dst"], key), src[np.argsort(top8, kind="stable")]), what
        assert np.array_equal(to_host(cb["counts"], "uint64").astype(np.int64), np.bincount(top8, minlength=256)), what
        for b, untouched in ((sb, ("src",) + st), (db, ()), (cb, ())):
            b.check("top level: " + what, untouched=untouched)
        kb, _ = _place("keys", src, 8, "random", 4)
        tb, _ = _place("tmp", (n, key), 0, "random", 5)
        c16, _ = _place("counts16", (65536, "uint64"), 8, "random", 6)
        _lib.check(lib.rdst_hip_split_top16_device(ctypes.c_void_p(kb["keys"].data_ptr()), ctypes.c_void_p(tb["tmp"].data_ptr()),
                                                   n, nbytes, kind_code, ctypes.c_void_p(c16["counts16"].data_ptr()), stream))
        gpu.device_status()
        assert same_bits(to_host(kb["keys"], key), src[np.argsort(top16, kind="stable")]), what
        assert np.array_equal(to_host(c16["counts16"], "uint64").astype(np.int64), np.bincount(top16, minlength=65536)), what
        for b in (kb, tb, c16):
            b.check("top 16: " + what)


# ---- host entry points ----------------------------------------------------------------------------------------------

def test_host_entries_stay_in_the_callers_array(gpu):
    """rdst_hip_sort and rdst_hip_sort_records on numpy views into a larger host array"""
    n = 100_003
    for key, off in (("uint32", 4), ("float64", 8), ("int16", 2), ("uint8", 3)):
        a = _random(n, key, n)
        for kind, fill in RUNS:
            k, exp = _case(kind, fill, a)
            hb, _ = _place("keys", k, off, _fill(fill, key), 1, device=None)
            gpu.sort_host_array(hb["keys"])
            what = f"host {key} {kind} fill={fill}"
            assert same_bits(hb["keys"], exp), what
            hb.check(what)
    rng = np.random.default_rng(0x5D570B40)
    # a u32 key field (naturally aligned inside 12-byte rows, as the entry requires) and a [u8; 20] one (26-byte rows, the
    # records at an odd byte offset)
    for N, ko, itemsize, base in ((4, 4, 12, 4), (20, 1, 26, 1)):
        dt = np.dtype({"names": ["tag", "k", "seq"], "formats": ["u1", "<u4" if N == 4 else ("u1", (N,)), "<u4"],
                       "offsets": [0, ko, itemsize - 4], "itemsize": itemsize})
        raw = np.zeros(n * dt.itemsize, dtype=np.uint8)
        rows = raw.reshape(n, dt.itemsize)
        keys = _byte_rows(rng, n, N)
        keys[1::3] = keys[0::3][: keys[1::3].shape[0]]          # equal keys that must keep their order
        rows[:, ko:ko + N] = keys
        rec = raw.view(dt)
        rec["seq"] = np.arange(n, dtype=np.uint32)
        order = np.argsort(rec["k"], kind="stable") if N == 4 else np.lexsort(keys.T[::-1])
        exp = rows[order].copy()
        hb, _ = _place("records", rec, base, "random", 2, device=None)
        gpu.sort_host_records(hb["records"], "k")
        assert np.array_equal(hb["records"].view(np.uint8).reshape(n, dt.itemsize), exp), N
        hb.check(f"records N={N}")


# ---- the round-1 sequence -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ("default", "atomic"))
def test_round_one_sequence(route, mode):
    """DESIGN.md §5, the round-1 abort: u32, u64, i32, i64 at 3 000 001 keys back to back on one stream, each keys and tmp
    0x100 after the end of the previous buffer (rounded to 256 bytes), all in one allocation; after every call the gaps,
    the keys still to be sorted and the results already checked must be as they were"""
    if mode == "atomic":
        route.set_hybrid(True, 1)
    n = 3_000_001
    keys = ("uint32", "uint64", "int32", "int64")
    inputs = {k: random_bits(n, k, 0x5D570B50 + i).copy() for i, k in enumerate(keys)}
    parts, pos = [], BAND_BYTES
    for k in keys:
        for name, init in ((f"keys_{k}", inputs[k]), (f"tmp_{k}", ((n,), k))):
            start = -(-pos // 256) * 256 + 0x100
            parts.append((name, init, start - pos))
            pos = start + n * np.dtype(k).itemsize
    arena = Bands(parts, seed=0x5D570B5F)
    done = []
    for i, k in enumerate(keys):
        route.sort_device_tensor(arena[f"keys_{k}"], arena[f"tmp_{k}"])
        r = route.last_route()
        assert mode == "default" or r == "atomic", (k, r)
        done.append(k)
        for d in done:
            assert same_bits(to_host(arena[f"keys_{d}"], d), reference_sorted(inputs[d])), (mode, k, d)
        arena.check(f"{mode}: after the {k} call", untouched=tuple(f"keys_{x}" for x in keys[i + 1:]))
