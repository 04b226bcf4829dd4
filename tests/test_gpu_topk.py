"""The partial sort (rdst_hip_topk_device) on the device.  Every case compares the keys — and the positions
where asked for — bit for bit with topk_inputs.expected_topk (a stable argsort by the mapped key), checks that the input is
unchanged and that what the device reports about its select (rdst_hip_debug_topk_state) equals the level loop restated in
numpy: the borders of the streaming kernels, every depth of the select at capacities on both sides of the bucket, ties
beyond the capacity (the keys-only fill, the position digits), inputs that put whole waves on one counter, float and signed
extremes, stream order, and guard bands around every buffer."""
import ctypes

import numpy as np
import pytest

import helpers as H
import topk_inputs as T

pytestmark = pytest.mark.gpu

POISON = 0xA5
SLACK = 4096     # poisoned bytes behind the scratch the call is told about


def _torch_index(index):
    import torch
    return {None: None, 4: torch.int32, 8: torch.int64}[index]


def _check(gpu, a, k, largest=False, index=None, cap=0, key=None, what="", keys_t=None, order=None):
    """one call on the keys `a` (numpy; `keys_t`: the device tensor that holds them, if the caller made it) and every
    comparison; returns the state"""
    import torch
    name = key if key else a.dtype.name
    t = H.to_device(np.ascontiguousarray(a)) if keys_t is None else keys_t
    need = gpu.topk_scratch_bytes(len(a), k, name, index or 0, cap)
    raw = torch.full((need + SLACK,), POISON, dtype=torch.uint8, device="cuda")
    ok, oi = gpu.topk_device_tensor(t, k, largest=largest, index=_torch_index(index), scratch=raw[:need], cand_capacity=cap, check=False, key=key)
    gpu.device_status()
    what = f"{what} {name} n = {len(a)} k = {k} largest = {largest} index = {index} cap = {cap}"
    if order is None:
        order = T.order_of(a, key, largest)
    ek, ei = a[order[:k]], order[:k].astype(np.int64)
    got = H.to_host(ok, a.dtype)
    assert got.shape == ek.shape and np.array_equal(got.view(np.uint8), ek.view(np.uint8)), what
    if index:
        assert oi.dtype == _torch_index(index) and np.array_equal(oi.cpu().numpy().astype(np.int64), ei), what
    else:
        assert oi is None
    assert np.array_equal(H.to_host(t, a.dtype).view(np.uint8), a.view(np.uint8)), what + ": the input changed"
    assert bool((raw[need:] == POISON).all()), what + ": written past scratch_bytes"
    state = gpu.topk_state(raw[:need])
    want = T.restate(a, k, largest, bool(index), cap, key)
    assert state == {f: want[f] for f in ("levels", "c_below", "candidates", "special")}, f"{what}: {state} != {want}"
    return state


# ---- 1: the borders of the streaming kernels ------------------------------------------------------------------------------

@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_every_key_type_at_the_streaming_borders(gpu, key, kb):
    wide = key if T.is_wide(key) else None
    for n in T.border_lengths(kb):
        a = T.random_keys(n, key, n + kb)
        if n > 8:
            a[n // 2:] = a[: n - n // 2]                                   # equal keys on both sides of any k
        for largest in (False, True):
            order = T.order_of(a, wide, largest)
            for k in T.ks_for(n):
                _check(gpu, a, k, largest, None, 64 if k % 2 else 0, wide, "border", order=order)
    # a key pointer with the element's alignment only, at a length with a head, a body and a tail
    n = T.block_batch(kb) + 2 * T.vec(kb) + 1
    big = T.random_keys(n + 1, key, 99)
    t = H.to_device(np.ascontiguousarray(big))
    for largest in (False, True):
        for k in (1, 65, n - 1):
            _check(gpu, big[1:], k, largest, None, 64, wide, "offset by one element", keys_t=t[1:])


@pytest.mark.parametrize("key,ib", T.INDEX_CASES, ids=[f"{k}-i{8 * ib}" for k, ib in T.INDEX_CASES])
def test_indexed_at_the_streaming_borders(gpu, key, ib):
    kb = T.key_bytes(key)
    for n in T.border_lengths(kb):
        a = T.random_keys(n, key, n + ib)
        if n > 8:
            a[n // 2:] = a[: n - n // 2]
        for largest in (False, True):
            order = T.order_of(a, None, largest)
            for k in T.ks_for(n):
                _check(gpu, a, k, largest, ib, 64 if k % 2 else 0, None, "indexed border", order=order)
    n = T.block_batch(kb) + 2 * T.vec(kb) + 1
    big = T.random_keys(n + 1, key, 98)
    t = H.to_device(big)
    for largest in (False, True):
        _check(gpu, big[1:], 65, largest, ib, 64, None, "offset by one element", keys_t=t[1:])


GRID = "one trip of the grid + 3"
LARGE = (("uint64", None, GRID), ("uint32", None, (1 << 22) + 5), ("float32", 4, (1 << 22) + 5), ("int64", 8, GRID), ("uint32", None, GRID))


@pytest.mark.parametrize("key,ib,n", LARGE, ids=[f"{k}-{ib}-{n}" for k, ib, n in LARGE])
def test_more_than_one_trip_of_the_grid(gpu, key, ib, n):
    import torch
    if n == GRID:                                                           # the grid is sized from the device's compute units
        n = T.grid_worth(T.key_bytes(key), torch.cuda.get_device_properties(0).multi_processor_count) + 3
    a = T.random_keys(n, key, 7)
    t = H.to_device(a)
    for largest in (False, True):
        order = T.order_of(a, None, largest)
        for k, cap in ((1, 0), (65, 64), (100_003, 0), (n - 1, 64)):          # (n - 1: every wave keeps more than one stage)
            st = _check(gpu, a, k, largest, ib, cap, None, "large", keys_t=t, order=order)
            assert st["levels"] >= 1


# ---- 2: every depth ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,j", T.depth_cases(), ids=[f"{d}-top{8 * j}" for d, j in T.depth_cases()])
def test_every_depth_at_capacities_around_the_bucket(gpu, dtype, j):
    kb = np.dtype(dtype).itemsize
    a = T.shared_top(T.DEPTH_LEN, dtype, j, 100 + j)
    t = H.to_device(a)
    k = T.DEPTH_LEN // 3
    m = T.restate(a, k, False, False, 64)["m"]
    depths = set()
    for cap in T.depth_capacities(m):
        for largest in (False, True):
            order = T.order_of(a, None, largest)
            depths.add(_check(gpu, a, k, largest, None, cap, None, f"top {8 * j} bits shared", keys_t=t, order=order)["levels"])
            if kb in (4, 8):
                _check(gpu, a, k, largest, 4 if j % 2 else 8, cap, None, f"top {8 * j} bits shared", keys_t=t, order=order)
    assert T.restate(a, k, False, False, 64)["levels"] in depths


@pytest.mark.parametrize("key,bits", T.wide_depth_cases(), ids=[f"{k}-top{b}" for k, b in T.wide_depth_cases()])
def test_every_depth_with_16_byte_keys(gpu, key, bits):
    """16-byte keys that share their top bits: the levels 2 to 11 of the select, the level whose digit straddles the two
    limbs (bits [56, 68)), the narrow last level, a 16-byte prefix in the pick, histogram and collection kernels, and — 120
    or 128 shared bits at a small capacity — the keys-only fill.  tests/test_topk_inputs.py holds the depth of every case."""
    a = T.wide_depth_input(key, bits)
    t = H.to_device(a)
    k = T.DEPTH_LEN // 3
    base = T.restate(a, k, False, False, 64, key)
    depths = set()
    for cap in T.depth_capacities(base["m"]):
        for largest in (False, True):
            order = T.order_of(a, key, largest)
            depths.add(_check(gpu, a, k, largest, None, cap, key, f"top {bits} bits shared", keys_t=t, order=order)["levels"])
    assert base["levels"] in depths
    if bits % 12 == 0 and bits <= 120:
        assert base["levels"] == bits // 12 + 1


@pytest.mark.parametrize("dtype,ib", T.FAR_CASES, ids=[f"{d}-i{8 * ib}" for d, ib in T.FAR_CASES])
def test_a_kth_element_beyond_position_2_to_the_20(gpu, dtype, ib):
    """All keys equal, with an index: the select runs through every position level, and the k-th element lies beyond
    position 2^20, so the top position digit (bits 20 to 31 of the position prefix and mask) is not 0 — in the histogram of
    the levels below it and in the collection's class of positions below the prefix.  The index must be 0 .. k - 1."""
    a = T.far_input(dtype)
    t = H.to_device(a)
    order = np.arange(T.FAR_LEN)
    for cap in T.FAR_CAPACITIES:
        for largest in (False, True):
            st = _check(gpu, a, T.FAR_K, largest, ib, cap, None, "far k", keys_t=t, order=order)
            assert st == {"levels": T.max_levels(a.dtype.itemsize, True), "c_below": T.FAR_K - 1, "candidates": 1, "special": 1}, st


# ---- 3: ties ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ("uint8", "int16", "uint32", "float32", "int64", "float64"))
def test_all_keys_equal_and_three_values(gpu, dtype):
    kb = np.dtype(dtype).itemsize
    n = 10_007
    for a in (np.full(n, H.random_bits(1, dtype, 3)[0], dtype=dtype), T.three_values(n, dtype, 5)):
        t = H.to_device(a)
        for largest in (False, True):
            order = T.order_of(a, None, largest)
            for k, cap in ((1, 1), (n // 2, 64), (n // 2, 0), (n - 1, 100), (n, 1)):
                st = _check(gpu, a, k, largest, None, cap, None, "equal keys", keys_t=t, order=order)
                if cap and len(np.unique(a)) == 1:
                    assert st["special"] == 1 and st["candidates"] == 0 and st["levels"] == T.key_levels(kb)
                if kb in (4, 8):
                    st = _check(gpu, a, k, largest, 4, cap, None, "equal keys", keys_t=t, order=order)
                    if cap:
                        assert st["special"] == 1 and st["levels"] > T.key_levels(kb) and 1 <= st["candidates"] <= cap


@pytest.mark.parametrize("dtype", ("uint32", "float32", "int64"))
def test_the_kth_key_tied_across_scattered_positions(gpu, dtype):
    a, k, at = T.tie_case(dtype, 3)
    t = H.to_device(a)
    order = T.order_of(a, None, False)
    below = int((H.mapped_key(a) < H.mapped_key(a[at[:1]])[0]).sum())
    assert np.array_equal(order[below:k], at[: k - below])                  # the lowest positions win
    for cap in (T.TIE_COUNT + 1, T.TIE_COUNT, T.TIE_COUNT - 1, 64, 1):
        fill = cap < T.TIE_COUNT
        st = _check(gpu, a, k, False, None, cap, None, "tie", keys_t=t, order=order)
        assert (st["candidates"] == 0 and st["special"] == 1) == fill
        for ib in (4, 8):
            st = _check(gpu, a, k, False, ib, cap, None, "tie", keys_t=t, order=order)
            assert st["special"] == int(fill) and 1 <= st["candidates"] <= cap
    # the largest k: the tie is met from the other side, the lowest positions still win
    order = T.order_of(a, None, True)
    above = int((H.mapped_key(a) > H.mapped_key(a[at[:1]])[0]).sum())
    kl = above + T.TIE_COUNT // 3
    assert np.array_equal(order[above:kl], at[: kl - above])
    for cap in (T.TIE_COUNT, 64):
        _check(gpu, a, kl, True, None, cap, None, "tie", keys_t=t, order=order)
        _check(gpu, a, kl, True, 8, cap, None, "tie", keys_t=t, order=order)


# ---- 4: whole waves on one counter ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", T.ORDER_FAMILIES)
def test_order_sensitive_inputs(gpu, name):
    for dtype, ib in (("uint32", None), ("float32", 4), ("uint64", 8), ("int64", None)):
        kb = np.dtype(dtype).itemsize
        n = 3 * T.block_batch(kb) + 17
        a = T.order_sensitive(name, n, dtype)
        t = H.to_device(a)
        for largest in (False, True):
            order = T.order_of(a, None, largest)
            for k, cap in ((1, 1), (n // 3, 64), (n // 3, 300), (n - 1, 0)):
                _check(gpu, a, k, largest, ib, cap, None, name, keys_t=t, order=order)


# ---- 5: floats and signed extremes ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ("float32", "float64"))
def test_float_specials(gpu, dtype):
    a = T.float_specials(dtype, 5000, 1)
    t = H.to_device(a)
    for largest in (False, True):
        order = T.order_of(a, None, largest)
        for k in (1, 2, 40, 400, 4999, 5000):
            for ib in (None, 4):
                _check(gpu, a, k, largest, ib, 64, None, "float specials", keys_t=t, order=order)


@pytest.mark.parametrize("dtype", ("int8", "int16", "int32", "int64"))
def test_signed_extremes(gpu, dtype):
    a = T.signed_extremes(dtype, 3000, 2)
    t = H.to_device(a)
    for largest in (False, True):
        order = T.order_of(a, None, largest)
        for k in (1, 10, 11, 1500, 2999, 3000):
            _check(gpu, a, k, largest, None, 16, None, "signed extremes", keys_t=t, order=order)
            if a.dtype.itemsize >= 4:
                _check(gpu, a, k, largest, 8, 16, None, "signed extremes", keys_t=t, order=order)


# ---- 6: stream order -----------------------------------------------------------------------------------------------------------

def test_stream_order(gpu):
    """on a stream of its own, keys written by a kernel enqueued just before the call; two calls back to back on one
    scratch with different inputs and no host step between them; check=False throughout, then ONE device_status"""
    import torch
    n, k = 200_003, 777
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        g = torch.Generator(device="cuda").manual_seed(11)
        need = max(gpu.topk_scratch_bytes(n, k, "int32", 8, 64), gpu.topk_scratch_bytes(n, 2 * k, "int32", 0, 64))
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        src = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device="cuda", generator=g)
        keys1 = torch.empty_like(src)
        keys1.copy_(src >> 7)                                               # written on this stream, just before the call
        k1, i1 = gpu.topk_device_tensor(keys1, k, index=torch.int64, scratch=scratch, cand_capacity=64, check=False)
        header1 = scratch[:256].clone()                                     # (a device copy, enqueued between the two calls)
        keys2 = src * 3 + 1
        k2, i2 = gpu.topk_device_tensor(keys2, 2 * k, largest=True, scratch=scratch, cand_capacity=64, check=False)
        state2 = gpu.topk_state(scratch)                                    # (blocking: after both calls were enqueued)
        state1 = gpu.topk_state(header1)
        gpu.device_status()
    a1, a2 = keys1.cpu().numpy(), keys2.cpu().numpy()
    ek, ei = T.expected_topk(a1, k)
    assert H.same_bits(k1.cpu().numpy(), ek) and np.array_equal(i1.cpu().numpy(), ei)
    ek2, _ = T.expected_topk(a2, 2 * k, largest=True)
    assert H.same_bits(k2.cpu().numpy(), ek2) and i2 is None
    want = T.restate(a2, 2 * k, True, False, 64)
    assert state2 == {f: want[f] for f in ("levels", "c_below", "candidates", "special")}
    want = T.restate(a1, k, False, True, 64)
    assert state1 == {f: want[f] for f in ("levels", "c_below", "candidates", "special")}


def test_no_wait_in_the_mode_that_splits_every_slice(gpu):
    """set_hybrid mode 17 makes rdst_hip_sort_device split — copy counts to the host and wait for the stream — at every
    length, as it does by itself from about 10^9 keys on.  The partial sort's k elements must not take that route: with
    50 ms of work queued in front of it the call returns while that work is still running, and the result is the same."""
    import torch
    n, k = 300_007, 70_001
    a = T.random_keys(n, "uint64", 31)
    b = T.random_keys(n, "float32", 32)
    ta, tb = H.to_device(a), H.to_device(b)
    sa = torch.empty(gpu.topk_scratch_bytes(n, k, "uint64", 0, 64), dtype=torch.uint8, device="cuda")
    sb = torch.empty(gpu.topk_scratch_bytes(n, k, "float32", 8, 64), dtype=torch.uint8, device="cuda")
    ballast = torch.zeros(1 << 28, dtype=torch.int32, device="cuda")
    gpu.set_hybrid("split_always")
    try:
        for timed in (False, True):                                         # (the first round grows the library's workspace)
            done = torch.cuda.Event()
            if timed:
                for _ in range(100):
                    ballast.add_(1)                                         # 2 GiB of traffic each: about 0.5 ms
            done.record()
            ka, _ = gpu.topk_device_tensor(ta, k, scratch=sa, cand_capacity=64, check=False)
            kb, ib = gpu.topk_device_tensor(tb, k, largest=True, index=torch.int64, scratch=sb, cand_capacity=64, check=False)
            returned_early = not done.query()
            gpu.device_status()
            assert returned_early or not timed, "the call waited for the stream"
        # the yardstick of this test: the sort entry in the same mode, behind the same work, does wait
        for _ in range(100):
            ballast.add_(1)
        done = torch.cuda.Event()
        done.record()
        gpu.sort_device_tensor(ta.clone(), check=False)
        assert done.query(), "mode 17 no longer makes rdst_hip_sort_device wait: this test shows nothing"
        gpu.device_status()
    finally:
        gpu.set_hybrid(True, 0)
    ea, _ = T.expected_topk(a, k)
    eb, ei = T.expected_topk(b, k, largest=True)
    assert H.same_bits(H.to_host(ka, "uint64"), ea)
    assert H.same_bits(H.to_host(kb, "float32"), eb) and np.array_equal(ib.cpu().numpy(), ei)


# ---- 7: bounds -------------------------------------------------------------------------------------------------------------------

def _raw_call(gpu, keys, n, k, out, idx, ib, scratch, sbytes, cap, kb, kind, flags):
    import torch
    from rdst_amd import _lib
    lib = _lib.load()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rdst_hip_topk_device(ctypes.c_void_p(keys.data_ptr()), n, k, ctypes.c_void_p(out.data_ptr()),
                                        ctypes.c_void_p(idx.data_ptr()) if idx is not None else None, ib, ctypes.c_void_p(scratch.data_ptr()), sbytes,
                                        cap, kb, kind, kb, flags, s))
    _lib.check(lib.rdst_hip_device_status(s))


BOUNDS = (("float32", 4, 4), ("int64", 8, 8), ("uint16", 0, 2), ("uint8", 0, 1), ("float64", 0, 8), ("uint32", 8, 12))


@pytest.mark.parametrize("dtype,ib,offset", BOUNDS, ids=[f"{d}-i{8 * ib}" for d, ib, _o in BOUNDS])
def test_every_buffer_stays_inside_its_bands(gpu, dtype, ib, offset):
    """keys at an element-aligned offset, both outputs with room behind k that must keep its poison, the scratch between bands
    and told its exact size"""
    kb = np.dtype(dtype).itemsize
    kind = gpu.key_info(dtype)[0]
    n = 2 * T.block_batch(kb) + 3 * T.vec(kb) + 1
    a = T.random_keys(n, dtype, 21)
    a[::3] = a[1]
    idt = {0: None, 4: "uint32", 8: "uint64"}[ib]
    for k, cap, largest in ((1, 1, False), (65, 64, True), (n // 2, 0, False), (n, 7, True)):
        need = gpu.topk_scratch_bytes(n, k, dtype, ib, cap)
        bk = H.banded(n, dtype, offset, seed=1, init=a)
        room = 100
        bo = H.banded(k + room, dtype, kb, seed=2, name="out")
        bi = H.banded(k + room, idt, ib, seed=3, name="index") if ib else None
        bs = H.banded(need, "uint8", 0, seed=4, name="scratch")
        out_before = H.to_host(bo["out"], dtype).copy()
        idx_before = H.to_host(bi["index"], idt).copy() if ib else None
        _raw_call(gpu, bk["keys"], n, k, bo["out"], bi["index"] if ib else None, ib, bs["scratch"], need, cap, kb, kind, 1 if largest else 0)
        ek, ei = T.expected_topk(a, k, largest)
        got = H.to_host(bo["out"], dtype)
        what = f"{dtype} k = {k} cap = {cap}"
        assert H.same_bits(got[:k], ek), what
        assert H.same_bits(got[k:], out_before[k:]), what + ": key output written beyond k"
        if ib:
            gi = H.to_host(bi["index"], idt)
            assert np.array_equal(gi[:k].astype(np.int64), ei), what
            assert np.array_equal(gi[k:], idx_before[k:]), what + ": index output written beyond k"
            bi.check(what)
        bk.check(what, untouched=("keys",))
        bo.check(what)
        bs.check(what)
        want = T.restate(a, k, largest, bool(ib), cap)
        assert gpu.topk_state(bs["scratch"]) == {f: want[f] for f in ("levels", "c_below", "candidates", "special")}, what
