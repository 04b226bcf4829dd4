"""The order statistics (rdst_hip_select_device) on the device.  Every case puts the input, both outputs and
the scratch into one poisoned arena, compares the keys — and the positions where asked for — bit for bit with
select_inputs.expected_select (a stable argsort by the mapped key), checks that every byte of the arena outside the output
slots and the scratch the call was told about is what it was (the input among them), and, where a case is named for a depth,
compares what the device reports (rdst_hip_debug_select_state) with the round loop restated in numpy."""
import ctypes

import numpy as np
import pytest

import helpers as H
import select_inputs as S
import topk_inputs as T

pytestmark = pytest.mark.gpu

POISON = 0xA5
SLACK = 4096     # poisoned bytes between and around the buffers


def _torch_index(index):
    import torch
    return {None: None, 4: torch.int32, 8: torch.int64}[index]


def _up(x, to):
    return (x + to - 1) // to * to


def _check(gpu, a, ranks, largest=False, index=None, cap=0, key=None, what="", mis=0, order=None, state=True):
    """one raw call on the keys `a` (`mis`: elements the key pointer stands behind a 16-byte boundary) and every comparison;
    returns the state of the last round"""
    import torch
    from rdst_amd import _lib
    lib = _lib.load()
    name = S.name_of(a, key)
    kind, kb, levels = gpu.key_info(name)
    n, nr = len(a), len(ranks)
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    need = gpu.select_scratch_bytes(n, nr, name, index or 0, cap)
    assert need > 0
    k_at = SLACK + 16 + mis * kb
    o_at = _up(k_at + raw.size + SLACK, 16)
    i_at = _up(o_at + nr * kb + SLACK, 16)
    s_at = _up(i_at + nr * (index or 0) + SLACK, 256)
    total = s_at + need + SLACK
    arena = torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 256 == 0
    arena[k_at:k_at + raw.size] = torch.from_numpy(raw.copy()).cuda()
    before = arena.cpu().numpy()
    base = arena.data_ptr()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.rdst_hip_select_device(ctypes.c_void_p(base + k_at), n, (ctypes.c_uint64 * nr)(*ranks), nr, ctypes.c_void_p(base + o_at),
                                    ctypes.c_void_p(base + i_at) if index else None, index or 0, ctypes.c_void_p(base + s_at), need, cap, kb, kind,
                                    levels, 1 if largest else 0, stream)
    _lib.check(rc)
    gpu.device_status()
    after = arena.cpu().numpy()
    what = f"{what} {name} n = {n} ranks = {list(ranks)[:6]}{'...' if nr > 6 else ''} largest = {largest} index = {index} cap = {cap} mis = {mis}"
    if order is None:
        order = T.order_of(a, key, largest)
    at = order[np.asarray(ranks, dtype=np.int64)]
    ek = np.ascontiguousarray(a[at]).view(np.uint8).reshape(-1)
    assert np.array_equal(after[o_at:o_at + nr * kb], ek), what
    if index:
        got = after[i_at:i_at + nr * index].view({4: np.uint32, 8: np.uint64}[index]).astype(np.int64)
        assert np.array_equal(got, at.astype(np.int64)), what
    untouched = before.copy()                                                # all but the slots and the scratch it was told about
    for lo, size in ((o_at, nr * kb), (i_at, nr * (index or 0)), (s_at, need)):
        untouched[lo:lo + size] = after[lo:lo + size]
    diff = np.nonzero(untouched != after)[0]
    assert diff.size == 0, f"{what}: bytes {diff[0]} .. {diff[-1]} of the arena changed (keys at {k_at}, outputs at {o_at}, {i_at}, scratch at {s_at})"
    st = gpu.select_state(arena[s_at:s_at + need])
    if state:
        want = S.restate_round(a, [r for r, _ in S.rounds_of(ranks)[-1]], largest, bool(index), cap, key)
        assert st == S.state_fields(want), f"{what}: {st} != {S.state_fields(want)}"
    return st


# ---- 1: the borders of the streaming kernels ------------------------------------------------------------------------------

@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_every_key_type_at_the_streaming_borders(gpu, key, kb):
    wide = key if T.is_wide(key) else None
    lengths = T.border_lengths(kb)
    for n in lengths:
        a = T.random_keys(n, key, n + kb)
        if n > 8:
            a[n // 2:] = a[: n - n // 2]                                   # equal keys around every rank
        for largest in (False, True):
            order = T.order_of(a, wide, largest)
            for j, ranks in enumerate(S.rank_sets(n)):
                _check(gpu, a, ranks, largest, None, 64 if j % 2 else 0, wide, "border", order=order)
    n = T.block_batch(kb) + 2 * T.vec(kb) + 1                              # a head, a body and a tail
    a = T.random_keys(n, key, 99)
    for largest in (False, True):
        for ranks in ([0, n - 1, n // 2], [n // 3]):
            _check(gpu, a, ranks, largest, None, 64, wide, "misaligned base", mis=1)


@pytest.mark.parametrize("key,ib", T.INDEX_CASES, ids=[f"{k}-i{8 * ib}" for k, ib in T.INDEX_CASES])
def test_indexed_at_the_streaming_borders(gpu, key, ib):
    kb = T.key_bytes(key)
    for n in T.border_lengths(kb):
        a = T.random_keys(n, key, n + ib)
        if n > 8:
            a[n // 2:] = a[: n - n // 2]
        for largest in (False, True):
            order = T.order_of(a, None, largest)
            for j, ranks in enumerate(S.rank_sets(n)):
                _check(gpu, a, ranks, largest, ib, 64 if j % 2 else 0, None, "indexed border", order=order)
    n = T.block_batch(kb) + 2 * T.vec(kb) + 1
    a = T.random_keys(n, key, 98)
    for largest in (False, True):
        _check(gpu, a, [0, n - 1, n // 2], largest, ib, 64, None, "misaligned base", mis=1)


LARGE = (("uint32", None), ("uint64", None), ("float32", 4))


@pytest.mark.parametrize("key,ib", LARGE, ids=[f"{k}-{ib}" for k, ib in LARGE])
def test_more_than_one_trip_of_the_grid(gpu, key, ib):
    import torch
    n = T.grid_worth(T.key_bytes(key), torch.cuda.get_device_properties(0).multi_processor_count) + 3
    a = T.random_keys(n, key, 7)
    order = T.order_of(a, None, False)
    st = _check(gpu, a, [0, n // 2, n - 1], False, ib, 0, None, "large", order=order, state=False)
    assert st["levels"] == 0 and st["candidates"] == n                       # below the default capacity: collected whole
    st = _check(gpu, a, S.spaced_ranks(n, 9) + [n - 1], False, ib, 4096, None, "large", order=order, state=False)
    assert st["levels"] >= 2 and st["groups"] == 10 and st["exhausted"] == 0
    st = _check(gpu, a, S.spaced_ranks(n, 9), True, ib, 1 << 16, None, "large", state=False)
    assert st["levels"] >= 1 and st["candidates"] <= 1 << 16


# ---- 2: groups ----------------------------------------------------------------------------------------------------------------

PARTING = [(dt, lv) for dt in ("uint32", "float64") for lv in (1, 2, S.key_levels(np.dtype(dt).itemsize) - 1)]


@pytest.mark.parametrize("dtype,level", PARTING, ids=[f"{d}-level{l}" for d, l in PARTING])
def test_two_ranks_that_part_at_a_level(gpu, dtype, level):
    a, ranks = S.parting_input(dtype, level, 40 + level)
    want = S.restate_round(a, ranks, False, False, 1)
    assert want["trace"][level - 1] == 1 and want["trace"][level] == 2
    m = S.restate_round(a, ranks, False, False, 64)["m"]
    ib = {"uint32": 4, "float64": 8}[dtype]
    for cap in S.capacities(m) + [S.DEPTH_LEN // 2 + 2000]:
        for largest in (False, True):
            rk = ranks if not largest else [S.DEPTH_LEN - 1 - r for r in reversed(ranks)]
            _check(gpu, a, rk, largest, None, cap, None, f"part at level {level}")
            _check(gpu, a, rk, largest, ib, cap, None, f"part at level {level}")


@pytest.mark.parametrize("dtype", ("uint32", "int64", "uint16"))
def test_max_ranks_in_distinct_buckets_and_in_one(gpu, dtype):
    ranks = S.spaced_ranks(S.DEPTH_LEN, S.MAX_RANKS)
    indexed = np.dtype(dtype).itemsize >= 4
    spread = T.random_keys(S.DEPTH_LEN, dtype, 61)
    one = S.one_bucket_input(dtype, 62)
    for a, name in ((spread, "distinct buckets"), (one, "one bucket")):
        first = S.restate_round(a, ranks, False, False, 1)["trace"]
        if np.dtype(dtype).itemsize >= 4:
            assert first[0] == (S.MAX_RANKS if name == "distinct buckets" else 1) and first[-1] == S.MAX_RANKS
        m = S.restate_round(a, ranks, False, False, 3 * S.MAX_RANKS)["m"]
        for cap in S.capacities(m):
            for largest in (False, True):
                _check(gpu, a, ranks, largest, None, cap, None, name)
            if indexed:
                _check(gpu, a, ranks, False, 4, cap, None, name)


@pytest.mark.parametrize("dtype", ("uint32", "float32", "int64"))
def test_one_heavy_group_beside_light_ones(gpu, dtype):
    a, ranks = S.heavy_input(dtype, 71)
    for cap in (1, 64, S.HEAVY_COUNT - 1, S.HEAVY_COUNT + 64, 0):
        for largest in (False, True):
            rk = ranks if not largest else [S.DEPTH_LEN - 1 - r for r in ranks]
            st = _check(gpu, a, rk, largest, None, cap, None, "heavy")
            if 0 < cap < S.HEAVY_COUNT:
                assert st["exhausted"] == 1 and st["candidates"] == 0
            _check(gpu, a, rk, largest, 8, cap, None, "heavy")


@pytest.mark.parametrize("count", (S.MAX_RANKS + 1, 2 * S.MAX_RANKS + 2))
def test_more_ranks_than_one_round_takes(gpu, count):
    """rounds in ascending rank order, results in the caller's slot order (the ranks come shuffled and with repeats)"""
    a = T.random_keys(S.DEPTH_LEN, "uint32", 81)
    a[::5] = a[2]
    rng = np.random.default_rng(count)
    ranks = S.spaced_ranks(S.DEPTH_LEN, count - 2) + [7, 7]
    ranks = [int(r) for r in rng.permutation(ranks)]
    assert len(S.rounds_of(ranks)) == -(-count // S.MAX_RANKS)
    for cap in (64, 0):
        _check(gpu, a, ranks, False, None, cap, None, "rounds")
        _check(gpu, a, ranks, True, 4, cap, None, "rounds")
    b = T.random_keys(S.DEPTH_LEN, "float64", 82)
    _check(gpu, b, ranks, False, 8, 64, None, "rounds")


# ---- 3: exhaustion -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ("uint8", "int16", "uint32", "float32", "int64", "float64"))
def test_all_keys_equal_and_three_values(gpu, dtype):
    kb = np.dtype(dtype).itemsize
    n = 10_007
    for a in (np.full(n, H.random_bits(1, dtype, 3)[0], dtype=dtype), T.three_values(n, dtype, 5)):
        for largest in (False, True):
            order = T.order_of(a, None, largest)
            for ranks, cap in (([0], 1), ([n // 2, n - 1, 0], 64), ([n // 2], 0), (S.spaced_ranks(n, 9), 100)):
                st = _check(gpu, a, ranks, largest, None, cap, None, "equal keys", order=order)
                if cap:
                    assert st == {"levels": S.key_levels(kb), "groups": len(np.unique(a[order[ranks]])), "candidates": 0, "exhausted": 1}
                if kb in (4, 8):
                    st = _check(gpu, a, ranks, largest, 4, cap, None, "equal keys", order=order)
                    if cap:                                                 # the position's digits are reached
                        assert st["levels"] > S.key_levels(kb)


@pytest.mark.parametrize("dtype", ("uint8", "int8"))
def test_one_byte_keys_where_level_0_is_the_whole_key(gpu, dtype):
    a = T.random_keys(S.DEPTH_LEN, dtype, 91)
    for largest in (False, True):
        st = _check(gpu, a, S.spaced_ranks(S.DEPTH_LEN, S.MAX_RANKS), largest, None, 64, None, "one byte")
        assert st["levels"] == 1 and st["exhausted"] == 1 and st["candidates"] == 0
        st = _check(gpu, a, [5, S.DEPTH_LEN - 1], largest, None, 0, None, "one byte")
        assert st["levels"] == 0 and st["candidates"] == S.DEPTH_LEN


@pytest.mark.parametrize("dtype,ib", (("uint16", None), ("uint32", None), ("uint32", 8), ("float64", None), ("int64", 4)))
def test_capacity_1_with_distinct_keys(gpu, dtype, ib):
    kb = np.dtype(dtype).itemsize
    a = H.unmapped(np.random.default_rng(5).permutation(S.DEPTH_LEN).astype(f"u{kb}") * (3 if kb > 2 else 1), dtype)
    for largest in (False, True):
        st = _check(gpu, a, [S.DEPTH_LEN // 2], largest, ib, 1, None, "capacity 1")
        assert st["groups"] == 1 and (st["candidates"] == 1 or st["exhausted"] == 1)
        _check(gpu, a, [0, 1, S.DEPTH_LEN - 1], largest, ib, 1, None, "capacity 1")


@pytest.mark.parametrize("key", T.WIDE_KEYS)
@pytest.mark.parametrize("bits", S.WIDE_BITS)
def test_16_byte_keys_that_share_their_top_bits(gpu, key, bits):
    a = T.shared_top_wide(S.DEPTH_LEN, key, bits, 300 + bits)
    ranks = [0, S.DEPTH_LEN // 3, S.DEPTH_LEN // 3 + 1, S.DEPTH_LEN - 1]
    for cap in (1, 64, 0):
        for largest in (False, True):
            st = _check(gpu, a, ranks, largest, None, cap, key, f"top {bits} bits shared")
            if bits == 128 and cap:
                assert st == {"levels": 16, "groups": 1, "candidates": 0, "exhausted": 1}
            if cap == 64 and bits in (60, 68):
                assert st["levels"] >= 1 + (bits - 12) // 8


# ---- 4: floats, signed extremes, ties --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_float_specials(gpu, dtype):
    a = T.float_specials(dtype, 5000, 1)
    order = T.order_of(a, None, False)
    special = np.nonzero(np.isnan(a) | np.isinf(a) | (a == 0))[0]
    inv = np.empty(len(a), dtype=np.int64)
    inv[order] = np.arange(len(a))
    ranks = sorted({int(r) for r in inv[special][:: max(len(special) // 40, 1)]} | {0, len(a) - 1})
    assert len(ranks) > 20
    for largest in (False, True):
        rk = ranks if not largest else [len(a) - 1 - r for r in ranks]
        for ib in (None, 4):
            for cap in (64, 0):
                _check(gpu, a, rk, largest, ib, cap, None, "float specials")


@pytest.mark.parametrize("dtype", ("int8", "int16", "int32", "int64"))
def test_signed_extremes(gpu, dtype):
    a = T.signed_extremes(dtype, 3000, 2)
    ranks = [0, 1, 9, 10, 11, 1499, 1500, 2988, 2989, 2990, 2998, 2999]
    for largest in (False, True):
        _check(gpu, a, ranks, largest, None, 16, None, "signed extremes")
        if a.dtype.itemsize >= 4:
            _check(gpu, a, ranks, largest, 8, 16, None, "signed extremes")


@pytest.mark.parametrize("dtype", ("uint32", "float32", "int64"))
def test_ranks_inside_a_run_of_ties_at_scattered_positions(gpu, dtype):
    a, k, at = T.tie_case(dtype, 3)
    below = int((H.mapped_key(a) < H.mapped_key(a[at[:1]])[0]).sum())
    ranks = [below, below + 1, k, below + T.TIE_COUNT - 1, below + 17]
    order = T.order_of(a, None, False)
    assert np.array_equal(order[below:below + T.TIE_COUNT], at)            # ascending positions within the run
    for cap in (T.TIE_COUNT, T.TIE_COUNT - 1, 64, 1):
        for ib in (4, 8):
            _check(gpu, a, ranks, False, ib, cap, None, "tie", order=order)
        _check(gpu, a, ranks, False, None, cap, None, "tie", order=order)
    above = int((H.mapped_key(a) > H.mapped_key(a[at[:1]])[0]).sum())
    _check(gpu, a, [above, above + 5, above + T.TIE_COUNT - 1], True, 8, 64, None, "tie")


# ---- 5: stream order and the wrapper ---------------------------------------------------------------------------------------------

def test_stream_order(gpu):
    """on a stream of its own, keys written by a kernel enqueued just before the call; two calls back to back on one
    scratch with different inputs and no host step between them; check=False throughout, then ONE device_status"""
    import torch
    n = 200_003
    r1, r2 = [0, n // 2, n - 1, n // 2], S.spaced_ranks(n, 70)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        g = torch.Generator(device="cuda").manual_seed(11)
        need = max(gpu.select_scratch_bytes(n, 4, "int32", 8, 64), gpu.select_scratch_bytes(n, 70, "int32", 0, 64))
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        src = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=g)
        keys1 = torch.empty_like(src)
        keys1.copy_(src >> 7)                                               # written on this stream, just before the call
        k1, i1 = gpu.select_device_tensor(keys1, r1, index=torch.int64, scratch=scratch, cand_capacity=64, check=False)
        header1 = scratch[:256].clone()                                     # (a device copy, enqueued between the two calls)
        keys2 = src * 3 + 1
        k2, i2 = gpu.select_device_tensor(keys2, r2, largest=True, scratch=scratch, cand_capacity=64, check=False)
        state2 = gpu.select_state(scratch)                                  # (blocking: after both calls were enqueued)
        state1 = gpu.select_state(header1)
        gpu.device_status()
    a1, a2 = keys1.cpu().numpy(), keys2.cpu().numpy()
    ek, ei = S.expected_select(a1, r1)
    assert H.same_bits(k1.cpu().numpy(), ek) and np.array_equal(i1.cpu().numpy(), ei)
    ek2, _ = S.expected_select(a2, r2, largest=True)
    assert H.same_bits(k2.cpu().numpy(), ek2) and i2 is None
    assert state2 == S.state_fields(S.restate(a2, r2, True, False, 64)[1][-1])
    assert state1 == S.state_fields(S.restate(a1, r1, False, True, 64)[1][-1])


def test_the_wrapper_s_arguments(gpu):
    import torch
    a = T.random_keys(5000, "float32", 4)
    t = H.to_device(a)
    ranks = S.spaced_ranks(5000, 9)
    for r in (ranks, np.array(ranks), torch.tensor(ranks)):
        k, i = gpu.select_device_tensor(t, r, index=torch.int32)
        ek, ei = S.expected_select(a, ranks)
        assert H.same_bits(H.to_host(k, "float32"), ek) and np.array_equal(i.cpu().numpy(), ei)
    with pytest.raises(ValueError, match="host"):
        gpu.select_device_tensor(t, torch.tensor(ranks).cuda())
    with pytest.raises(ValueError):
        gpu.select_device_tensor(t, [5000])
    k, i = gpu.select_device_tensor(t, [])
    assert k.numel() == 0 and i is None
    w = T.random_keys(3000, "u128", 5)
    k, _ = gpu.select_device_tensor(H.to_device(w), [0, 2999, 1500], largest=True, key="u128")
    assert np.array_equal(k.cpu().numpy().view(np.uint64), S.expected_select(w, [0, 2999, 1500], True, "u128")[0])
    assert gpu.quantile_ranks(5000, [0.5], "lower") == [2499]


def test_no_blocking_call_without_check(gpu):
    """with 50 ms of work queued in front of it the call returns while that work is still running — at a capacity that takes
    every level, with an index, and over more than one round — and the result is the same"""
    import torch
    n = 300_007
    a = T.random_keys(n, "uint64", 31)
    b = T.three_values(n, "float32", 32)
    ta, tb = H.to_device(a), H.to_device(b)
    ra, rb = S.spaced_ranks(n, 70), [0, n // 2, n - 1]
    sa = torch.empty(gpu.select_scratch_bytes(n, 70, "uint64", 0, 64), dtype=torch.uint8, device="cuda")
    sb = torch.empty(gpu.select_scratch_bytes(n, 3, "float32", 8, 64), dtype=torch.uint8, device="cuda")
    ballast = torch.zeros(1 << 28, dtype=torch.int32, device="cuda")
    gpu.set_hybrid("split_always")
    try:
        for timed in (False, True):                                         # (the first round grows the library's workspace)
            done = torch.cuda.Event()
            if timed:
                for _ in range(100):
                    ballast.add_(1)                                         # 2 GiB of traffic each: about 0.5 ms
            done.record()
            ka, _ = gpu.select_device_tensor(ta, ra, scratch=sa, cand_capacity=64, check=False)
            kb, ib = gpu.select_device_tensor(tb, rb, largest=True, index=torch.int64, scratch=sb, cand_capacity=64, check=False)
            returned_early = not done.query()
            gpu.device_status()
            assert returned_early or not timed, "the call waited for the stream"
    finally:
        gpu.set_hybrid(True, 0)
    ea, _ = S.expected_select(a, ra)
    eb, ei = S.expected_select(b, rb, largest=True)
    assert H.same_bits(H.to_host(ka, "uint64"), ea)
    assert H.same_bits(H.to_host(kb, "float32"), eb) and np.array_equal(ib.cpu().numpy(), ei)
