"""rdst_hip_search_device on the MI355X: every comparison exact, against numpy on the host
(tests/search_inputs.py: np.searchsorted over the mapped keys, Python integers for 16-byte keys).  The haystack, the needles,
both outputs and the scratch sit between poisoned bands in one allocation; slots the call must not write hold a pattern that
is compared afterwards."""
import numpy as np
import pytest

import helpers as H
import runs_inputs as R
import search_inputs as S

pytestmark = pytest.mark.gpu

RDST_ERR_DEVICE = -5
BAND = 64 << 10
SIDES = ("left", "right", "both")


def _np_dtype(key):
    return np.dtype(np.uint64) if S.wide(key) else np.dtype(key)


def _tensor(view, key):
    """the Bands view as the tensor the wrapper takes: 128-bit keys as (n, 2) int64 limbs"""
    import torch
    return view.view(torch.int64) if S.wide(key) else view


def _host(t):
    import torch
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(it).cpu().numpy()


def _bits_of(t, key):
    a = _host(t)
    return a.view(np.uint64) if S.wide(key) else a.view(f"u{a.dtype.itemsize}")


def _device(keys, key):
    """a numpy key array as the tensor the wrappers take"""
    import torch
    if S.wide(key):
        return torch.from_numpy(keys.view(np.int64).copy()).cuda()
    return H.to_device(keys)


def _part(a, key):
    """a Bands part for the keys `a` (an empty view needs its shape spelled out)"""
    return a if len(a) else (((0, 2) if S.wide(key) else (0,)), _np_dtype(key))


def run_case(gpu, hay, needles, key, what, side="both", off="int64", m=None, length=None, want=None, gap=0, expect_error=None, same=False):
    """one call in guarded buffers, everything it may and may not write compared; returns search_state.  `want`: the
    (lower, upper) of S.expected if the caller has them already, "range": only that every output lies in [0, m].  `same`: the
    needles ARE the haystack (one tensor).  `gap`: extra bytes in front of the needles (a base aligned to the element only)."""
    kb = S.key_bytes(key)
    n, nn = len(hay), len(needles)
    m = n if m is None else m
    ob = np.dtype(off).itemsize
    sbytes = gpu.search_scratch_bytes(n, nn, key)
    if want is None and m <= n:
        want = S.expected(hay, needles, key, m)
    pos = BAND + n * kb
    gaps = []
    for nbytes, align, extra in ((nn * kb, 16, gap), ((nn + 3) * ob, 8, 0), ((nn + 3) * ob, 8, 0), (sbytes, 256, 0)):
        if same and not gaps:                                                 # no view of their own
            gaps.append(0)
            continue
        gaps.append((-pos) % align + align + extra)
        pos += gaps[-1] + nbytes
    parts = [("hay", _part(hay, key), 0)]
    if not same:
        parts.append(("needles", _part(needles, key), gaps[0]))
    parts += [("lower", np.full(nn + 3, -1, dtype=off), gaps[1]), ("upper", np.full(nn + 3, -1, dtype=off), gaps[2]), ("scratch", ((sbytes,), np.uint8), gaps[3])]
    bands = H.Bands(parts, band_bytes=BAND, seed=n + nn)
    assert bands["scratch"].data_ptr() % 256 == 0 and bands["lower"].data_ptr() % 8 == 0 and bands["upper"].data_ptr() % 8 == 0
    hay_t = _tensor(bands["hay"], key)
    needles_t = hay_t if same else _tensor(bands["needles"], key)
    assert same or needles_t.data_ptr() % 16 == gap % 16
    lower_t, upper_t = bands["lower"][:nn], bands["upper"][:nn]
    out = (lower_t, upper_t) if side == "both" else lower_t if side == "left" else upper_t
    got = gpu.search_device_tensor(hay_t, needles_t, side=side, length=length, positions=off, scratch=bands["scratch"], check=False,
                                   key=key if S.wide(key) else None, out=out)
    first = got[0] if side == "both" else got
    assert first.data_ptr() == (upper_t if side == "right" else lower_t).data_ptr()
    if expect_error:
        with pytest.raises(gpu.RdstHipError) as e:
            gpu.device_status()
        assert e.value.code == RDST_ERR_DEVICE and f"= 0x{expect_error:x} (" in str(e.value), str(e.value)
    gpu.device_status()                                                       # clean, or raised once and clean again
    state = gpu.search_state(bands["scratch"])
    g_lower, g_upper = _host(bands["lower"]), _host(bands["upper"])
    for name, g, wanted, idx in (("lower", g_lower, side != "right", 0), ("upper", g_upper, side != "left", 1)):
        e = np.full(nn + 3, -1, dtype=off)
        if wanted and m <= n and isinstance(want, str):
            u = g[:nn].view(f"u{ob}")
            assert np.all(u <= m), (what, name, int(u.max()), m)             # some position in [0, m]
            e[:nn] = g[:nn]
        elif wanted and m <= n:
            e[:nn] = want[idx].astype(f"u{ob}").view(off)                     # (4-byte positions past 2^31: the same bits)
        assert np.array_equal(g, e), (what, name, np.flatnonzero(g != e)[:8], g[g != e][:8], e[g != e][:8])
    bands.check(what, untouched=("hay",) if same else ("hay", "needles"))
    assert state["m"] == m and state["past"] == (1 if m > n else 0)
    if m <= n and m > 0 and nn > 0:
        assert state["staged"] + state["table"] == -(-nn // S.tile(kb)), (what, state)
    else:
        assert state["staged"] == state["table"] == 0, (what, state)
    return state


@pytest.mark.parametrize("key,kb", S.KEY_CASES)
def test_every_width_and_kind_at_every_border(gpu, key, kb):
    """case 1: the haystack lengths round the splitter table and the window, the needle counts round the tile; left, right and
    both; 4- and 8-byte positions; present keys, keys in between, below the first, above the last, the extremes; and once a
    needle base that is aligned to the element only (the loads key by key)"""
    assert gpu.search_limits(key) == (S.tile(kb), S.SPLITTERS, S.WINDOW[kb])
    cases = 0
    for m in S.haystack_lengths(kb):
        hay = S.haystack(key, m, seed=kb)
        for nn in S.needle_counts(kb):
            needles = S.needles_for(hay, key, nn, seed=m)
            want = S.expected(hay, needles, key)
            for side in SIDES:
                for off in ("int32", "int64"):
                    run_case(gpu, hay, needles, key, f"{key}: m = {m}, {nn} needles, {side}, {off}", side=side, off=off, want=want)
                    cases += 1
            if kb < 16 and nn == 3 * S.tile(kb) + 5:
                run_case(gpu, hay, needles, key, f"{key}: m = {m}, needle base aligned to the element only", want=want, gap=kb)
    assert cases == 10 * 5 * 6                                                   # none left out: the share of skipped cases is 0


def test_float_keys_go_by_their_bits(gpu):
    """case 2: -0.0 and +0.0, and each NaN, are separate keys for both sides"""
    for name, (hay, needles, lower, upper) in S.float_cases().items():
        want = (np.array(lower), np.array(upper))
        assert [w.tolist() for w in S.expected(hay, needles, name)] == [lower, upper]
        for side in SIDES:
            run_case(gpu, hay, needles, name, f"{name}: {side}", side=side, want=want)
        # the same keys many times over, so that runs of each of them cross the window and the splitters
        reps = S.WINDOW[hay.dtype.itemsize] // 4 + 3
        big = np.repeat(hay, reps)
        run_case(gpu, big, needles, name, f"{name}: every key {reps} times", want=(want[0] * reps, want[1] * reps))
        run_case(gpu, big, np.tile(needles, 200), name, f"{name}: every key {reps} times, tiles of needles")


@pytest.mark.parametrize("key", ("uint8", "float32", "int64", "u128"))
def test_ties(gpu, key):
    """case 3: a haystack that is all one key; a run of equal keys longer than the window that covers several splitters;
    needles below, at and above the key, sorted (the staged path wherever the tile's stretch fits) and shuffled; upper - lower
    is the run's length"""
    kb = S.key_bytes(key)
    t, w = S.tile(kb), S.WINDOW[kb]
    m = 3 * w + 5
    hay = S.haystack(key, m, seed=3, distinct=1)
    for nn in (1, t + 1):
        needles = S.needles_for(hay, key, nn, seed=4)
        needles[0] = hay[0]
        lower, upper = S.expected(hay, needles, key)
        assert lower[0] == 0 and upper[0] == m and set((upper - lower).tolist()) <= {0, m}
        for side in SIDES:
            run_case(gpu, hay, needles, key, f"{key}: all one key, {nn} needles, {side}", side=side, off="int32", want=(lower, upper))
    run_case(gpu, hay, hay[:t], key, f"{key}: all one key, a tile of that key")
    if kb == 1:
        return
    m, start, length = 8 * w, 3 * w + 17, w + 7                                  # splitters every 8 W / 1 024 keys: the run covers hundreds
    assert m // S.SPLITTERS * 3 < length
    hay = S.ramp(key, m, plateau=(start, length))
    img = [int(x) for x in S.mapped(hay[[start - 1, start, start + length]], key)]
    near = S.from_mapped([img[0], img[0] + 1, img[1] - 1, img[1], img[1] + 1, img[2] - 1, img[2]], key)
    pick = np.random.default_rng(kb).integers(0, m, size=t + 1 - len(near))
    needles = np.concatenate([near, hay[pick]])
    order = np.argsort(np.concatenate([np.arange(len(near)) * 0 + start, pick]), kind="stable")
    for name, q in (("shuffled", needles), ("sorted", needles[order])):
        lower, upper = S.expected(hay, q, key)
        at = np.flatnonzero(lower == start)
        assert len(at) and np.all(upper[at][(upper - lower)[at] > 0] == start + length)
        state = run_case(gpu, hay, q, key, f"{key}: a run of {length} keys, {name} needles", want=(lower, upper))
        assert state["table"] >= 1                                               # (a tile that holds the run's key spans more than the window)


@pytest.mark.parametrize("key", ("uint32", "float64", "u128"))
def test_both_paths(gpu, key):
    """case 4: the same needles sorted and dealt out across the tiles give the same answer per needle; sorted they take the
    staged path in every tile (a tile's T neighbouring keys span T <= W keys of the haystack), dealt out the table path in
    every tile (a tile spans all but 7 of the 8 T > W keys); a tile's stretch of exactly W keys is staged, W + 1 is not; the
    first and the last key in one tile take the table path"""
    kb = S.key_bytes(key)
    t, s, w = gpu.search_limits(key)
    tiles = 8
    m, nn = 8 * w, tiles * t
    assert t <= w and nn <= m - 5 and nn - tiles + 1 > w
    hay = S.ramp(key, m)
    needles = hay[5:5 + nn]
    lower, upper = S.expected(hay, needles, key)
    assert lower.tolist() == list(range(5, 5 + nn)) and np.all(upper == lower + 1)
    state = run_case(gpu, hay, needles, key, f"{key}: sorted needles", want=(lower, upper))
    assert state == {"m": m, "staged": tiles, "table": 0, "past": 0}
    deal = S.interleaved(nn, tiles)
    state = run_case(gpu, hay, needles[deal], key, f"{key}: needles dealt out", want=(lower[deal], upper[deal]))
    assert state == {"m": m, "staged": 0, "table": tiles, "past": 0}
    for last, staged in ((w - 1, 1), (w, 0)):                                    # [lower(min), upper(max)) holds last + 1 keys
        ends = hay[[100, 100 + last]]
        state = run_case(gpu, hay, ends, key, f"{key}: a stretch of {last + 1} keys")
        assert (state["staged"], state["table"]) == (staged, 1 - staged)
        inside = np.concatenate([ends, hay[100:100 + last:7]])
        state = run_case(gpu, hay, inside, key, f"{key}: a stretch of {last + 1} keys, needles inside")
        assert (state["staged"], state["table"]) == (staged, 1 - staged)
    state = run_case(gpu, hay, hay[[0, m - 1]], key, f"{key}: the first and the last key")
    assert (state["staged"], state["table"]) == (0, 1)


@pytest.mark.parametrize("key", ("uint32", "u128"))
def test_more_tiles_than_can_be_resident_at_once(gpu, key):
    """case 5: 2^20 keys, 2^22 + 3 needles: 2 049 (u128: 4 097) tiles of needles.  The u128 needles are drawn from 2^14 distinct
    ones, whose positions the Python-integer statement gives once"""
    import torch
    m, nn = 1 << 20, (1 << 22) + 3
    rng = np.random.default_rng(5)
    if S.wide(key):
        hay = rng.integers(0, 1 << 64, size=(m, 2), dtype=np.uint64, endpoint=False)
        hay[:, 1] >>= np.uint64(50)                                               # high limbs repeat: the low limb decides often
        hay = H.wide_sorted(hay, key)
        pool = np.concatenate([hay[rng.integers(0, m, size=1 << 13)], rng.integers(0, 1 << 64, size=(1 << 13, 2), dtype=np.uint64, endpoint=False) >> np.uint64(25)])
        pool_lower, pool_upper = S.expected(hay, pool, key)
        pick = rng.integers(0, len(pool), size=nn)
        needles, lower, upper = pool[pick], pool_lower[pick], pool_upper[pick]
    else:
        hay = np.sort(rng.integers(0, 1 << 32, size=m, dtype=np.uint64).astype(np.uint32) & np.uint32(0xFFFFFFFE))
        needles = rng.integers(0, 1 << 32, size=nn, dtype=np.uint64).astype(np.uint32)
        needles[::3] = hay[rng.integers(0, m, size=len(needles[::3]))]
        lower, upper = S.expected(hay, needles, key)
    assert np.any(upper > lower) and np.any(upper == lower)
    for positions in ("int64", "int32"):
        got_lower, got_upper = gpu.search_device_tensor(_device(hay, key), _device(needles, key), side="both", positions=positions,
                                                        key=key if S.wide(key) else None)
        assert got_lower.dtype == getattr(torch, positions) and len(got_lower) == nn
        assert np.array_equal(_host(got_lower), lower) and np.array_equal(_host(got_upper), upper)


@pytest.mark.parametrize("key", ("uint8", "int32", "uint64", "u128"))
def test_length_on_the_device(gpu, key):
    """case 6: m below len with unsorted garbage behind it, which must not matter; an int32 and an int64 length; m > len
    writes not one byte, sets bit 0x20, and device_status raises once"""
    import torch
    kb = S.key_bytes(key)
    t, s, w = gpu.search_limits(key)
    n = 3 * w + 5 + 100
    hay = S.haystack(key, n, seed=6)
    tail = np.random.default_rng(kb).permutation(n - 2 * w) + 2 * w               # everything behind 2 W in disorder
    hay[2 * w:] = hay[tail]
    needles = S.needles_for(hay[:2 * w], key, t + 1, seed=7)
    for m in (0, 1, s - 1, s + 1, w, w + 1, 2 * w):
        want = S.expected(hay, needles, key, m)
        for dtype in ("int32", "int64"):
            length = torch.tensor([m], dtype=getattr(torch, dtype), device="cuda")
            run_case(gpu, hay, needles, key, f"{key}: m = {m}, {dtype}", m=m, length=length, want=want, side="both" if m % 2 else "left")
    good = S.haystack(key, n, seed=8)
    for m in (n + 1, 1 << 31, (1 << 32) + 5):
        length = torch.tensor([m], dtype=torch.int64, device="cuda")
        run_case(gpu, good, needles, key, f"{key}: m = {m} > len", m=m, length=length, expect_error=S.ERR_LEN_PAST_CAPACITY)
    run_case(gpu, good, needles, key, f"{key}: valid right after")


def test_a_length_written_on_the_stream_just_before(gpu):
    """the length is produced by a torch kernel enqueued just before the call on the same non-default stream"""
    import torch
    t, s, w = gpu.search_limits("uint32")
    n = 3 * w + 5
    hay = S.haystack("uint32", n, seed=9)
    m = w + 3
    needles = S.needles_for(hay[:m], "uint32", 2 * t + 1, seed=10)
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    flags[:m] = 1
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        length = flags.sum(dtype=torch.int64).reshape(1)                        # a reduction kernel on `side`; never read here
        run_case(gpu, hay, needles, "uint32", "length from a reduction on a side stream", m=m, length=length)
    side.synchronize()
    assert int(length.item()) == m


@pytest.mark.parametrize("key", ("uint8", "int32", "float32", "uint64", "u128"))
def test_sort_runs_and_search_without_the_host(gpu, key):
    """case 7: sort, runs, then the distinct keys searched for the original keys with length = n_runs: unique[inverse] == keys
    bit for bit, with ONE look at the device status at the end; unique_device_tensor(inverse=True) the same way"""
    import torch
    rng = np.random.default_rng(77)
    n = 50000
    wide_key = key if S.wide(key) else None
    if S.wide(key):
        pool = rng.integers(0, 1 << 64, size=(700, 2), dtype=np.uint64, endpoint=False)
        pool[:, 1] &= np.uint64(3)
        keys = pool[rng.integers(0, 700, size=n)]
    else:
        keys = H.random_bits(700, key, 5)[rng.integers(0, 700, size=n)].copy()
    d = _device(keys, key)
    before = d.clone()
    work = d.clone()
    gpu.sort_device_tensor(work, check=False, key=wide_key)
    uniq, _starts, count = gpu.runs_device_tensor(work, starts=None, check=False, key=wide_key)
    inverse = gpu.search_device_tensor(uniq, d, side="left", length=count, check=False, key=wide_key)
    gpu.device_status()
    runs = int(count.item())
    bits = R.bits(keys)
    assert runs == len(np.unique(bits, axis=0)) and inverse.dtype == torch.int64
    inv = _host(inverse)
    assert inv.min() == 0 and inv.max() == runs - 1
    assert np.array_equal(_bits_of(uniq, key)[inv], bits) and np.array_equal(_host(d), _host(before))
    for counts in (False, True):
        got = gpu.unique_device_tensor(d, counts=counts, key=wide_key, inverse=True)
        plain = gpu.unique_device_tensor(d, counts=counts, key=wide_key)
        assert len(got) == len(plain) + 1 and int(got[-2].item()) == runs == int(plain[-1].item())
        for a, b in zip(got[:-2], plain[:-1]):
            assert np.array_equal(_host(a[:runs]), _host(b[:runs]))
        assert got[-1].dtype == torch.int64 and np.array_equal(_host(got[-1]), inv)
        assert np.array_equal(_bits_of(got[0], key)[_host(got[-1])], bits)
    assert np.array_equal(_host(d), _host(before))


@pytest.mark.parametrize("key", ("int16", "float32", "u128"))
def test_needles_that_are_the_haystack_itself(gpu, key):
    """case 8: ONE tensor as both inputs: lower and upper are each element's group borders, equal to what runs says"""
    kb = S.key_bytes(key)
    m = 3 * S.WINDOW[kb] + 5
    hay = S.haystack(key, m, seed=11)
    _run_keys, starts, runs = R.expected(hay)
    group = np.cumsum(R.heads_of(hay)) - 1
    borders = np.r_[starts, m]
    want = (borders[group], borders[group + 1])
    assert [w.tolist() for w in S.expected(hay, hay, key)] == [w.tolist() for w in want] and runs < m
    state = run_case(gpu, hay, hay, key, f"{key}: searched for its own keys", want=want, same=True)
    assert state["table"] == 0                                                    # sorted needles: every tile staged
    r_keys, r_starts, r_count = gpu.runs_device_tensor(_device(hay, key), key=key if S.wide(key) else None)
    assert int(r_count.item()) == runs and np.array_equal(_host(r_starts[:runs + 1]), borders)


@pytest.mark.parametrize("key", ("uint8", "float32", "uint64", "u128"))
def test_an_unsorted_haystack_costs_correctness_only(gpu, key):
    """case 9: one shuffled array of 3 W + 5 keys: every output in [0, m], the bands intact, the call ends"""
    kb = S.key_bytes(key)
    m = 3 * S.WINDOW[kb] + 5
    hay = S.haystack(key, m, seed=12, distinct=m)
    hay = hay[np.random.default_rng(13).permutation(m)]
    needles = S.needles_for(hay[:0], key, 3 * S.tile(kb) + 5, seed=14)
    for side in SIDES:
        for off in ("int32", "int64"):
            run_case(gpu, hay, needles, key, f"{key}: unsorted, {side}, {off}", side=side, off=off, want="range")
    run_case(gpu, hay, np.sort(hay.reshape(m, -1), axis=0).reshape(hay.shape)[:S.tile(kb)], key, f"{key}: unsorted, clustered needles", want="range")


def test_position_arithmetic_past_2_31(gpu):
    """case 10: 3 * 2^30 one-byte keys holding the values 0 ... 191 in order, 2^24 of each (arange(m) >> 24: the shift that
    gives 192 values; a shift of 22 would give 768, which wrap in a byte and are not sorted).  The 256 byte values are the
    needles; both sides; 4- and 8-byte positions; the expected positions in closed form"""
    import torch
    m, each = 3 << 30, 1 << 24
    hay = torch.empty(m, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for a in range(0, m, step):
        hay[a:a + step] = (torch.arange(a, a + step, dtype=torch.int64, device="cuda") >> 24).to(torch.uint8)
    assert int(hay[-1].item()) == 191 and int(hay[each].item()) == 1 and int(hay[each - 1].item()) == 0
    values = np.arange(256, dtype=np.int64)
    lower, upper = np.minimum(values, 192) * each, np.minimum(values + 1, 192) * each
    assert upper[191] == m and lower[129] > (1 << 31) and upper.max() < (1 << 32)
    needles = torch.arange(256, dtype=torch.int64, device="cuda").to(torch.uint8)
    scratch = torch.empty(gpu.search_scratch_bytes(m, 256, "uint8"), dtype=torch.uint8, device="cuda")
    for positions, view in (("int64", np.uint64), ("int32", np.uint32)):
        out = torch.full((2, 256 + 8), -1, dtype=getattr(torch, positions), device="cuda")
        got = gpu.search_device_tensor(hay, needles, side="both", positions=positions, scratch=scratch, out=(out[0, :256], out[1, :256]))
        for g, want in zip(got, (lower, upper)):
            assert np.array_equal(_host(g).view(view).astype(np.int64), want)
        assert bool((out[:, 256:] == -1).all())
        assert gpu.search_state(scratch) == {"m": m, "staged": 0, "table": 1, "past": 0}
        # one value per call: [lower, upper) is 2^24 keys, the table path, at positions past 2^31
        one = torch.full((300,), 150, dtype=torch.uint8, device="cuda")
        lo150, up150 = gpu.search_device_tensor(hay, one, side="both", positions=positions, scratch=scratch)
        assert np.all(_host(lo150).view(view) == 150 * each) and np.all(_host(up150).view(view) == 151 * each)
