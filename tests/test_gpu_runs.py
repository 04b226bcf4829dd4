"""rdst_hip_runs_device on the MI355X: every comparison exact, against numpy on the host
(tests/runs_inputs.py: heads = r_[True, bits[1:] != bits[:-1]], then keys[heads], flatnonzero(heads), heads.sum()).  The
inputs, the input's copy and every output sit between poisoned bands in one allocation; slots the call must not write hold a
pattern that is compared afterwards."""
import numpy as np
import pytest

import helpers as H
import runs_inputs as R

pytestmark = pytest.mark.gpu

RDST_ERR_DEVICE = -5
BAND = 64 << 10          # four tiles on each side of every view
POISON = 0xA5


def _np_dtype(key):
    return np.dtype(np.uint64) if R.wide(key) else np.dtype(key)


def _tensor(view, key):
    """the Bands view as the tensor the wrapper takes: 128-bit keys as (n, 2) int64 limbs"""
    import torch
    return view.view(torch.int64) if R.wide(key) else view


def _host(t):
    import torch
    it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().view(it).cpu().numpy()


def _bits_of(t, key):
    """a device tensor's bits as numpy unsigned integers ((n, 2) uint64 limbs for 128-bit keys)"""
    a = _host(t)
    return a.view(np.uint64) if R.wide(key) else a.view(f"u{a.dtype.itemsize}")


def _length(m, dtype):
    import torch
    return None if dtype is None else torch.tensor([m], dtype=getattr(torch, dtype), device="cuda")


def run_case(gpu, keys, key, what, m=None, length_dtype=None, capacity=None, off="int64", pad=False, run_keys=True, starts=True, gap=0, expect_error=None,
             length=None):
    """one call in guarded buffers, everything it may and may not write compared; returns R"""
    import torch
    n = len(keys)
    m = n if m is None else m
    capacity = n if capacity is None else capacity
    kb = 16 if R.wide(key) else keys.dtype.itemsize
    ob = np.dtype(off).itemsize
    kdt = _np_dtype(key)
    want_keys, want_starts, runs = R.expected(keys, min(m, n))
    kept = min(runs, capacity)
    out_shape = (capacity + 3, 2) if R.wide(key) else (capacity + 3,)
    sbytes = gpu.runs_scratch_bytes(n, key)
    # the views one behind the other, each after a gap that aligns it: the outputs to 8 bytes (keys of 16: to 16), the scratch to 256
    pos = BAND + gap + n * kb
    gaps = []
    for nbytes, align in (((capacity + 3) * kb, max(kb, 8)), ((capacity + 4) * ob, 8), (3 * ob, 8), (sbytes, 256)):
        gaps.append((-pos) % align + align)
        pos += gaps[-1] + nbytes
    bands = H.Bands([("keys", keys if n else ((0, 2) if R.wide(key) else (0,), kdt), gap),
                     ("out", np.full(out_shape, POISON * 0x0101010101010101 & ((1 << (8 * kdt.itemsize)) - 1), dtype=f"u{kdt.itemsize}"), gaps[0]),
                     ("starts", np.full(capacity + 4, -1, dtype=off), gaps[1]),
                     ("count", np.full(3, -1, dtype=off), gaps[2]),
                     ("scratch", ((sbytes,), np.uint8), gaps[3])], band_bytes=BAND, seed=n + capacity)
    assert bands["scratch"].data_ptr() % 256 == 0 and bands["starts"].data_ptr() % 8 == 0 and bands["out"].data_ptr() % kb == 0
    keys_t = _tensor(bands["keys"], key)
    out = (bands["out"].view(keys_t.dtype)[:capacity] if run_keys else None, bands["starts"][:capacity + 1] if starts else None, bands["count"][:1])
    if length is None:
        length = _length(m, length_dtype)
    got = gpu.runs_device_tensor(keys_t, length=length, capacity=capacity, starts=off if starts else None, pad=pad, scratch=bands["scratch"],
                                 check=False, key=key if R.wide(key) else None, out=out)
    assert got[2].data_ptr() == bands["count"].data_ptr()
    if expect_error is None and capacity and runs > capacity:
        expect_error = R.ERR_RUNS_TRUNCATED
    if expect_error:
        with pytest.raises(gpu.RdstHipError) as e:
            gpu.device_status()
        assert e.value.code == RDST_ERR_DEVICE and f"= 0x{expect_error:x} (" in str(e.value), str(e.value)
    gpu.device_status()                                                       # clean, or raised once and clean again
    g_out, g_starts, g_count = _bits_of(bands["out"], key), _host(bands["starts"]), _host(bands["count"])
    poison_key = np.uint64(POISON * 0x0101010101010101 & ((1 << (8 * kdt.itemsize)) - 1)).astype(g_out.dtype)
    e_out = np.full(g_out.shape, poison_key, dtype=g_out.dtype)
    e_starts = np.full(capacity + 4, -1, dtype=off)
    e_count = np.full(3, -1, dtype=off)
    if m <= n:
        e_count[0] = runs
        if capacity and run_keys:
            e_out[:kept] = R.bits(want_keys)[:kept]
        if capacity and starts:
            e_starts[:kept] = want_starts[:kept]
            e_starts[kept] = want_starts[capacity] if runs > capacity else m    # the end of the last kept run
            if pad and runs <= capacity:
                e_starts[runs:capacity + 1] = m
    assert np.array_equal(g_count, e_count), (what, g_count, e_count)
    assert np.array_equal(g_starts, e_starts), (what, np.flatnonzero(g_starts != e_starts)[:8], runs, capacity)
    assert np.array_equal(g_out, e_out), (what, np.flatnonzero((g_out != e_out).reshape(len(e_out), -1).any(axis=1))[:8], runs, capacity)
    bands.check(what, untouched=("keys",))
    return runs


@pytest.mark.parametrize("key,kb", R.KEY_CASES)
def test_every_width_and_kind_at_every_border(gpu, key, kb):
    """case 1: the lengths round the tile, heads on both sides of a tile border, tiles without a head, a walk longer than the
    look-back window; both offset widths; a key base that is aligned to the element only (the loads key by key)"""
    t, window = gpu.runs_limits(key)
    assert (t, window) == (R.tile(kb), R.LOOKBACK_WINDOW)
    for i, (name, heads) in enumerate(R.shapes(kb).items()):
        keys = R.keys_from_heads(heads, key, seed=i)
        for off in ("int64", "int32"):
            runs = run_case(gpu, keys, key, f"{key}: {name}, {off}", off=off)
            assert runs == int(heads.sum())
        if kb < 16 and len(keys) > t:
            run_case(gpu, keys, key, f"{key}: {name}, base aligned to the element only", gap=kb)


def test_float_keys_go_by_their_bits(gpu):
    for name, (keys, starts) in R.float_cases().items():
        assert run_case(gpu, keys, keys.dtype.name, name) == len(starts)


def test_keys_that_differ_in_one_half_only(gpu):
    heads = R.random_runs(3 * R.tile(8) + 5, np.random.default_rng(1), 3)
    for name, key, half in R.half_cases():
        assert run_case(gpu, R.keys_from_heads(heads, key, half=half), key, name) == int(heads.sum())


def _plain_call(gpu, keys, key=None, **kw):
    import torch
    t = torch.from_numpy(keys.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[keys.dtype.itemsize])).cuda()
    t = t if key else t.view(getattr(torch, keys.dtype.name))
    return gpu.runs_device_tensor(t, key=key, **kw)


@pytest.mark.parametrize("key,n", (("uint32", (1 << 23) + 3), ("uint8", 1 << 23), ("uint8", 1 << 24)))
@pytest.mark.parametrize("long_run", (False, True))
def test_more_tiles_than_can_be_resident_at_once(gpu, key, n, long_run):
    """case 2: runs of random length 1 .. 9, and the same with one run of 3 T + 1 keys in the middle.  With 8-byte starts the u32
    kernel holds 282 registers (one workgroup on each of the 256 compute units, against 513 tiles) and the u8 kernel 234 (two
    workgroups: 512 at once — exactly the 512 tiles of 2^23 keys, so 2^24 keys, 1 024 tiles, are run as well)"""
    t = R.tile(np.dtype(key).itemsize)
    heads = R.random_runs(n, np.random.default_rng([n, long_run]))
    if long_run:
        mid = n // 2 + 7
        heads[mid + 1:mid + 3 * t + 1] = False
    keys = R.keys_from_heads(heads, key)
    want_keys, want_starts, runs = R.expected(keys)
    assert runs == int(heads.sum()) and (not long_run or (np.diff(want_starts) >= 3 * t + 1).any())
    got_keys, got_starts, got_count = _plain_call(gpu, keys, capacity=runs + 5, pad=True)
    assert int(got_count.item()) == runs
    assert np.array_equal(_host(got_keys[:runs]).view(keys.dtype), want_keys)
    assert np.array_equal(_host(got_starts[:runs]), want_starts) and np.all(_host(got_starts[runs:]) == n)


@pytest.mark.parametrize("key", ("uint8", "float32", "u128"))
def test_guard_bands_and_padding(gpu, key):
    """case 3: slots behind R untouched without PAD, exactly (R, capacity] equal to m with it; the input unchanged (run_case
    compares every byte round and between the buffers)"""
    kb = 16 if R.wide(key) else np.dtype(key).itemsize
    heads = R.random_runs(2 * R.tile(kb) + 77, np.random.default_rng(kb))
    keys = R.keys_from_heads(heads, key)
    runs = int(heads.sum())
    for pad in (False, True):
        for off in ("int32", "int64"):
            for capacity in (runs, runs + 1, runs + 1500, len(keys)):
                assert run_case(gpu, keys, key, f"{key}: capacity {capacity}, pad {pad}, {off}", capacity=capacity, pad=pad, off=off) == runs
    run_case(gpu, keys[:0], key, f"{key}: no key at all, padded", capacity=9, pad=True)


@pytest.mark.parametrize("key", ("int16", "uint32", "float64", "i128"))
def test_capacity(gpu, key):
    """case 4: R - 1 (truncated: the first R - 1 runs complete, the true count, RDST_ERR_DEVICE once, then clean), R, 0 with NULL
    outputs (count only, no error), keys only, starts only"""
    kb = 16 if R.wide(key) else np.dtype(key).itemsize
    heads = R.random_runs(3 * R.tile(kb) + 5, np.random.default_rng(kb + 40))
    keys = R.keys_from_heads(heads, key)
    runs = int(heads.sum())
    for off in ("int32", "int64"):
        for pad in (False, True):                                               # (a truncated table is never padded)
            assert run_case(gpu, keys, key, f"{key}: capacity R - 1", capacity=runs - 1, off=off, pad=pad, expect_error=R.ERR_RUNS_TRUNCATED) == runs
        run_case(gpu, keys, key, f"{key}: capacity 1", capacity=1, off=off, expect_error=R.ERR_RUNS_TRUNCATED)
        run_case(gpu, keys, key, f"{key}: capacity R", capacity=runs, off=off)
        run_case(gpu, keys, key, f"{key}: counting call", capacity=0, off=off, run_keys=False, starts=False)
        run_case(gpu, keys, key, f"{key}: counting call with outputs", capacity=0, off=off)
        run_case(gpu, keys, key, f"{key}: keys only", off=off, starts=False)
        run_case(gpu, keys, key, f"{key}: starts only", off=off, run_keys=False, pad=True)
        run_case(gpu, keys, key, f"{key}: starts only, truncated", capacity=runs // 2, off=off, run_keys=False)
        run_case(gpu, keys, key, f"{key}: keys only, truncated", capacity=runs // 2, off=off, starts=False)


@pytest.mark.parametrize("key", ("uint8", "int32", "uint64", "u128"))
def test_length_on_the_device(gpu, key):
    """case 5: m at each border under a fixed capacity with an int32 and an int64 length; a tail of distinct keys that would
    add runs if it were read; m > len writes nothing and reports 0x20 once"""
    kb = 16 if R.wide(key) else np.dtype(key).itemsize
    t = R.tile(kb)
    n = 3 * t + 5 + 100
    heads = R.random_runs(n, np.random.default_rng(kb + 50))
    heads[3 * t + 5:] = True                                                     # the tail: every key a run of its own
    keys = R.keys_from_heads(heads, key)
    for m in R.border_lengths(t) + (n,):
        for length_dtype in ("int32", "int64"):
            runs = run_case(gpu, keys, key, f"{key}: m = {m}, {length_dtype}", m=m, length_dtype=length_dtype, capacity=n, pad=(m % 2 == 0))
            assert runs == int(heads[:m].sum())
    for m in (n + 1, 1 << 31, (1 << 32) + 5):
        run_case(gpu, keys, key, f"{key}: m = {m} > len", m=m, length_dtype="int64", capacity=n, pad=True, expect_error=R.ERR_LEN_PAST_CAPACITY)
    run_case(gpu, keys, key, f"{key}: valid right after", capacity=n)


def test_a_length_written_on_the_stream_just_before(gpu):
    """the length is produced by a torch kernel enqueued just before the call on the same non-default stream"""
    import torch
    t = R.tile(4)
    n = 5 * t + 9
    heads = R.random_runs(n, np.random.default_rng(60))
    keys = R.keys_from_heads(heads, "uint32")
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    m = 2 * t + 3
    flags[:m] = 1
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        length = flags.sum(dtype=torch.int64).reshape(1)                        # a reduction kernel on `side`; never read here
        runs = run_case(gpu, keys, "uint32", "length from a reduction on a side stream", m=m, capacity=n, pad=True, length=length)
    side.synchronize()
    assert runs == int(heads[:m].sum()) and int(length.item()) == m


def test_sort_group_and_median_of_every_group_without_the_host(gpu):
    """case 6: sort (key, row id) pairs, runs with pad at a capacity of 1 024, the median of every group by the segmented
    select over 1 024 segments; empty groups' slots unwritten; ONE look at the device status, at the end"""
    import torch
    rng = np.random.default_rng(66)
    n, distinct = 20000, 300
    pool = rng.choice(1 << 20, size=distinct, replace=False).astype(np.uint32)
    keys = pool[rng.integers(0, distinct, size=n)]
    values = rng.standard_normal(n).astype(np.float32)
    d_keys = H.to_device(keys)
    rows = torch.arange(n, dtype=torch.int32, device="cuda")
    gpu.sort_pairs_device_tensor(d_keys, rows, check=False)
    run_keys, starts, count = gpu.runs_device_tensor(d_keys, capacity=1024, pad=True, check=False)
    grouped = H.to_device(values)[rows.long()]                                  # a torch gather: the values in group order
    out = torch.full((1024, 1), float("nan"), dtype=torch.float32, device="cuda")
    medians, _ = gpu.select_segments_device_offsets_tensor(grouped, starts, quantiles=[0.5], far_capacity=0, check=False, out=(out, None))
    gpu.device_status()
    uniq, cnt = np.unique(keys, return_counts=True)
    assert len(uniq) == distinct == int(count.item())
    assert np.array_equal(_host(run_keys[:distinct]).view(np.uint32), uniq)
    assert np.array_equal(_host(starts), np.r_[0, np.cumsum(cnt), np.full(1024 - distinct, n)])
    got = medians.cpu().numpy().reshape(-1)
    for g, k in enumerate(uniq):
        group = np.sort(values[keys == k])
        assert got[g] == group[(len(group) - 1) // 2], (g, k)                   # numpy's "lower" median
    assert np.isnan(got[distinct:]).all()                                        # empty groups: not written


@pytest.mark.parametrize("key", ("uint8", "int32", "float32", "uint64", "u128"))
def test_unique_device_tensor(gpu, key):
    """case 7: against np.unique on the bit view in the sort's order, with counts"""
    import torch
    rng = np.random.default_rng(77)
    n = 50000
    if R.wide(key):
        pool = rng.integers(0, 1 << 64, size=(700, 2), dtype=np.uint64, endpoint=False)
        pool[:, 1] &= np.uint64(3)
        keys = pool[rng.integers(0, 700, size=n)]
        order = np.lexsort((keys[:, 0], keys[:, 1]))
        srt = keys[order]
        d = torch.from_numpy(keys.view(np.int64)).cuda()
    else:
        dt = np.dtype(key)
        pool = H.random_bits(700, key, 5)
        keys = pool[rng.integers(0, 700, size=n)].copy()
        srt = keys[np.argsort(H.mapped_key(keys), kind="stable")]
        d = H.to_device(keys)
    before = d.clone()
    want_keys, want_starts, runs = R.expected(srt)
    want_counts = np.diff(np.r_[want_starts, n])
    uniq, counts, count = gpu.unique_device_tensor(d, counts=True, key=key if R.wide(key) else None)
    assert int(count.item()) == runs and np.array_equal(_host(d), _host(before))              # (the bits: random floats hold NaNs)
    assert np.array_equal(_bits_of(uniq[:runs], key), R.bits(want_keys))
    assert np.array_equal(_host(counts), np.r_[want_counts, np.zeros(n - runs, dtype=np.int64)])
    if not R.wide(key):
        u = keys.view(f"u{keys.dtype.itemsize}")
        assert runs == len(np.unique(u)) and sorted(_bits_of(uniq[:runs], key).tolist()) == np.unique(u).tolist()
    uniq2, count2 = gpu.unique_device_tensor(d, key=key if R.wide(key) else None)
    assert int(count2.item()) == runs and np.array_equal(_bits_of(uniq2[:runs], key), R.bits(want_keys))
