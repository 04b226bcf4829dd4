"""The segmented partial sort (rdst_hip_topk_segments_device) on the device.  Every case compares the WHOLE
output buffers — guard bands, rows, and the slots from k_s on, all pre-filled — bit for bit with the numpy statement
(topk_segments_inputs.expected_rows: per segment the first k_s of a stable argsort by the mapped key), and checks that the
input is unchanged and that nothing was written before or behind the scratch the call was told about."""
import numpy as np
import pytest

import helpers as H
import topk_inputs as T
import topk_segments_inputs as S

pytestmark = pytest.mark.gpu

POISON = 0xA5
SLACK = 4096     # poisoned bytes before and behind the scratch the call is told about (a multiple of its 256-byte alignment)
GUARD = 64       # pre-filled elements before and behind each output
FILL_KEY = 0x5A  # every byte of a pre-filled key slot
FILL_INDEX = -7


def _torch_index(ib):
    import torch
    return {None: None, 4: torch.int32, 8: torch.int64}[ib]


class Table:
    """keys on the device and a table of borders, with what does not depend on k computed once"""

    def __init__(self, a, off, key=None):
        self.a, self.off, self.key = np.ascontiguousarray(a), np.asarray(off, dtype=np.uint64), key
        self.name = key if key else a.dtype.name
        self.t = H.to_device(self.a)
        self.n_seg = len(self.off) - 1
        self.longest = int((self.off[1:] - self.off[:-1]).max()) if self.n_seg else 0
        self._ordered = {}

    def ordered(self, largest):
        if largest not in self._ordered:
            self._ordered[largest] = S.table_order(self.a, self.off, largest, self.key)
        return self._ordered[largest]


def _call(gpu, tb, k, largest, ib, scratch=None):
    """enqueues one call (check=False) on pre-filled, guarded outputs; returns what _verify needs"""
    import torch
    per_key = 2 if T.is_wide(tb.key) else 1
    slots = tb.n_seg * k
    raw_k = torch.full(((slots + 2 * GUARD) * per_key * tb.a.dtype.itemsize,), FILL_KEY, dtype=torch.uint8, device="cuda")
    out_k = raw_k.view(tb.t.dtype)[GUARD * per_key:(GUARD + slots) * per_key]
    raw_i = out_i = None
    if ib:
        raw_i = torch.full((slots + 2 * GUARD,), FILL_INDEX, dtype=_torch_index(ib), device="cuda")
        out_i = raw_i[GUARD:GUARD + slots]
    need = gpu.topk_segments_scratch_bytes(tb.n_seg, tb.longest, k, tb.name, ib or 0)
    if scratch is not None:                                                 # shared by several calls: the bands lie round the largest need
        assert scratch.numel() >= need + 2 * SLACK
        need = scratch.numel() - 2 * SLACK
    raw_s = scratch if scratch is not None else torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
    got = gpu.topk_segments_device_tensor(tb.t, tb.off, k, largest=largest, index=_torch_index(ib), scratch=raw_s[SLACK:SLACK + need], check=False,
                                          key=tb.key, out=(out_k, out_i))
    assert got[0] is out_k and got[1] is out_i
    return raw_k, raw_i, raw_s, need


def _verify(gpu, tb, k, largest, ib, bufs, what=""):
    raw_k, raw_i, raw_s, need = bufs
    gpu.device_status()
    what = f"{what} {tb.name} segments = {tb.n_seg} k = {k} largest = {largest} index = {ib}"
    per_key = 2 if T.is_wide(tb.key) else 1
    want_k = np.full((tb.n_seg * k + 2 * GUARD) * per_key * tb.a.dtype.itemsize, FILL_KEY, dtype=np.uint8).view(tb.a.dtype)
    rows_k = want_k[GUARD * per_key:(GUARD + tb.n_seg * k) * per_key].reshape((tb.n_seg, k, 2) if per_key == 2 else (tb.n_seg, k))
    want_i = np.full(tb.n_seg * k + 2 * GUARD, FILL_INDEX, dtype=np.int64)
    S.expected_rows(tb.a, tb.off, k, largest, tb.key, rows_k, want_i[GUARD:GUARD + tb.n_seg * k].reshape(tb.n_seg, k), tb.ordered(largest))
    got_k = raw_k.cpu().numpy()
    if not np.array_equal(got_k, want_k.view(np.uint8).reshape(-1)):
        bad = np.flatnonzero(got_k != want_k.view(np.uint8).reshape(-1))
        slot = int(bad[0]) // (per_key * tb.a.dtype.itemsize) - GUARD
        raise AssertionError(f"{what}: keys differ in {len(bad)} bytes, first in row {slot // k} slot {slot % k} "
                             f"(segment of {int(tb.off[slot // k + 1] - tb.off[slot // k]) if 0 <= slot < tb.n_seg * k else '?'} keys)")
    if ib:
        got_i = raw_i.cpu().numpy().astype(np.int64)
        if not np.array_equal(got_i, want_i):
            slot = int(np.flatnonzero(got_i != want_i)[0]) - GUARD
            raise AssertionError(f"{what}: positions differ, first in row {slot // k} slot {slot % k}: {got_i[slot + GUARD]} != {want_i[slot + GUARD]}")
    assert np.array_equal(H.to_host(tb.t, tb.a.dtype).view(np.uint8), tb.a.view(np.uint8)), what + ": the input changed"
    assert bool((raw_s[:SLACK] == POISON).all()) and bool((raw_s[SLACK + need:] == POISON).all()), what + ": written outside the scratch"


def _check(gpu, tb, k, largest=False, ib=None, what=""):
    _verify(gpu, tb, k, largest, ib, _call(gpu, tb, k, largest, ib), what)


@pytest.fixture
def stream_max(gpu):
    """the setter, put back to the default afterwards"""
    yield gpu.set_topk_segments_stream_max
    gpu.set_topk_segments_stream_max(0)


# ---- 1: every length at every start, every k, every key type ----------------------------------------------------------------

def _length_table(gpu, key, ib):
    kb = T.key_bytes(key)
    wm, bm, _sm, _ksm = gpu.topk_segments_limits(key, ib or 0)
    assert (wm, bm) == (S.wave_max(kb), S.block_max(kb, bool(ib)))
    off, n = S.residue_table(S.segment_lengths(wm, bm), kb)
    return Table(S.keys_for(n, key, 11 + kb), off, key if T.is_wide(key) else None), wm, bm


@pytest.mark.parametrize("key,kb", T.KEY_TYPES, ids=[k for k, _ in T.KEY_TYPES])
def test_every_length_start_and_k_keys_only(gpu, key, kb):
    tb, wm, bm = _length_table(gpu, key, None)
    for k in S.table_ks(wm, bm):
        for largest in (False, True):
            _check(gpu, tb, k, largest, None, "lengths")


@pytest.mark.parametrize("key,ib", T.INDEX_CASES, ids=[f"{k}-i{8 * ib}" for k, ib in T.INDEX_CASES])
def test_every_length_start_and_k_with_an_index(gpu, key, ib):
    tb, wm, bm = _length_table(gpu, key, ib)
    for k in S.table_ks(wm, bm):
        for largest in (False, True):
            _check(gpu, tb, k, largest, ib, "lengths")


# ---- 2: the stream class: depth, stop rule, ties -----------------------------------------------------------------------------

DEPTH_DTYPES = ("uint16", "int32", "float32", "uint64", "float64")


@pytest.mark.parametrize("dtype", DEPTH_DTYPES)
def test_stream_class_at_every_depth(gpu, dtype):
    """segments of 2 bm + 3 keys whose mapped keys share their top 0, 12, 24 ... bits, up to all of them: the select takes 1,
    2, 3 ... levels (tests/test_topk_segments_inputs.py holds the depth of every segment), starts of three residues"""
    kb = np.dtype(dtype).itemsize
    for ib in ((None, 4) if kb == 4 else (None, 8) if kb == 8 else (None,)):
        bm = gpu.topk_segments_limits(dtype, ib or 0)[1]
        n = 2 * bm + 3
        parts = [S.shared_digits(n, dtype, j, 40 + j) for j in range(T.key_levels(kb) + 1)]
        off = np.cumsum([1] + [n] * len(parts)).astype(np.uint64)
        a = np.concatenate([parts[0][:1]] + parts + [parts[0][:2]])
        tb = Table(a, off)
        for k in (1, bm // 2 + 1, bm):
            for largest in (False, True):
                _check(gpu, tb, k, largest, ib, "depth")


@pytest.mark.parametrize("dtype,ib", (("uint32", None), ("float32", 8), ("int64", 4), ("uint16", None)))
def test_stop_rule_border(gpu, dtype, ib):
    """c_below + m exactly TILE after the first level: the select stops; TILE + 1: it takes a second level"""
    bm = gpu.topk_segments_limits(dtype, ib or 0)[1]
    n = 2 * bm + 3
    for extra in (0, 1):
        a, k = S.stop_border(dtype, bm, n, extra, 5 + extra)
        assert S.stream_depth(a, k, False, bm)[0] == 1 + extra
        tb = Table(np.concatenate([a[:3], a]), np.array([3, 3 + n], dtype=np.uint64))
        for largest in (False, True):
            _check(gpu, tb, k, largest, ib, f"stop rule, TILE + {extra}")


@pytest.mark.parametrize("dtype,ib", (("uint32", 4), ("float64", 8), ("uint8", None), ("int16", None), ("u128", None)))
def test_ties_in_the_stream_class(gpu, dtype, ib):
    key = dtype if T.is_wide(dtype) else None
    bm = gpu.topk_segments_limits(dtype, ib or 0)[1]
    n = 2 * bm + 3
    one = T.random_keys(1, dtype, 9)
    equal = np.repeat(one, n, axis=0)                                       # digits exhausted with more than TILE ties
    if key:
        three = T.random_keys(3, dtype, 10)[np.random.default_rng(1).integers(0, 3, size=n)]
    else:
        three = T.three_values(n, dtype, 10)
    tb = Table(np.concatenate([one, equal, three]), np.array([1, 1 + n, 1 + 2 * n], dtype=np.uint64), key)
    for k in (1, 2, bm - 1, bm):
        for largest in (False, True):
            _check(gpu, tb, k, largest, ib, "ties")


@pytest.mark.parametrize("dtype,ib", (("uint32", 4), ("int32", 8), ("float64", 4)))
def test_scattered_ties_take_the_lowest_positions(gpu, dtype, ib):
    bm = gpu.topk_segments_limits(dtype, ib)[1]
    n = 3 * bm + 5
    a, k, t_at = S.scattered_ties(dtype, n, bm, 21)
    tb = Table(np.concatenate([a[:2], a]), np.array([2, 2 + n], dtype=np.uint64))
    bufs = _call(gpu, tb, k, False, ib)
    _verify(gpu, tb, k, False, ib, bufs, "scattered ties")
    got = bufs[1].cpu().numpy()[GUARD:GUARD + k].astype(np.int64)
    below = bm // 4
    assert np.array_equal(got[below:], t_at[:k - below]), "the ties that win are the first in position order"
    _check(gpu, tb, k, True, ib, "scattered ties")


# ---- 3: whole tables -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,ib", (("uint32", None), ("float32", 4), ("uint64", 8), ("int8", None), ("i128", None)))
def test_one_table_with_all_four_classes(gpu, stream_max, dtype, ib):
    key = dtype if T.is_wide(dtype) else None
    kb = T.key_bytes(dtype)
    wm, bm = gpu.topk_segments_limits(dtype, ib or 0)[:2]
    off, n, sm = S.mixed_table(wm, bm, 3)
    stream_max(sm)
    assert gpu.topk_segments_limits(dtype, ib or 0) == (wm, bm, sm, bm)
    tb = Table(S.keys_for(n, dtype, 31), off, key)
    for k in (1, 77, bm):
        items, counts, longest_far = gpu.topk_segments_plan(off, n, k, dtype, ib or 0)
        assert all(c > 0 for c in counts) and longest_far == 4 * bm + 7
        assert (items, counts, longest_far) == S.plan(off, k, kb, bool(ib), sm)
        for largest in (False, True):
            _check(gpu, tb, k, largest, ib, "four classes")


def test_wave_class_grid_beyond_one_trip(gpu):
    rng = np.random.default_rng(8)
    off = np.cumsum(np.concatenate([[2], rng.integers(1, 4, size=70_000)])).astype(np.uint64)
    tb = Table(T.three_values(int(off[-1]) + 1, "uint32", 4), off)
    for k, largest, ib in ((1, False, None), (2, True, 8), (3, False, 4)):
        _check(gpu, tb, k, largest, ib, "70 000 short segments")


def test_many_block_class_workgroups(gpu):
    wm = gpu.topk_segments_limits("float32", 4)[0]
    off = (np.arange(5_001, dtype=np.uint64) * np.uint64(wm + 1)) + np.uint64(1)
    tb = Table(S.keys_for(int(off[-1]), "float32", 6), off)
    _check(gpu, tb, 5, True, 4, "5 000 block-class segments")
    _check(gpu, tb, wm + 1, False, None, "5 000 block-class segments")


def test_rows_of_a_matrix(gpu):
    import torch
    a = S.keys_for(37 * 1000, "float32", 12).reshape(37, 1000)
    t = H.to_device(a.reshape(-1)).reshape(37, 1000)
    keys, index = gpu.topk_rows_tensor(t, 10, largest=True, index=torch.int64)
    want_k = np.zeros((37, 10), dtype=np.float32)
    want_i = np.zeros((37, 10), dtype=np.int64)
    S.expected_rows(a.reshape(-1), np.arange(38) * 1000, 10, True, None, want_k, want_i)
    assert keys.shape == (37, 10) and np.array_equal(H.to_host(keys, np.float32).view(np.uint32), want_k.view(np.uint32))
    assert np.array_equal(index.cpu().numpy(), want_i)


# ---- 4: stream and far class agree; stream order --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,ib", (("uint32", None), ("float32", 4), ("int64", 8), ("uint16", None)))
def test_stream_and_far_class_give_the_same_bits(gpu, stream_max, dtype, ib):
    bm = gpu.topk_segments_limits(dtype, ib or 0)[1]
    off = np.cumsum([1, bm + 1, 2 * bm + 3, 0, bm + 1025]).astype(np.uint64)
    tb = Table(S.keys_for(int(off[-1]) + 2, dtype, 17), off)
    for k in (1, 65, bm):
        for largest in (False, True):
            outs = []
            for border in (bm, 0):
                stream_max(border)
                assert gpu.topk_segments_plan(off, len(tb.a), k, dtype, ib or 0)[1] == ((0, 0, 0, 3) if border else (0, 0, 3, 0))
                bufs = _call(gpu, tb, k, largest, ib)
                _verify(gpu, tb, k, largest, ib, bufs, f"stream_max = {border}")
                outs.append(bufs)
            assert bool((outs[0][0] == outs[1][0]).all()) and (not ib or bool((outs[0][1] == outs[1][1]).all()))


def test_behind_a_kernel_that_writes_the_keys(gpu):
    import torch
    bm = gpu.topk_segments_limits("uint32", 4)[1]
    off, n = S.residue_table([1, 65, 600, bm + 1, 2 * bm + 3], 4)
    a = S.keys_for(n, "uint32", 23)
    tb = Table(np.zeros_like(a), off)
    src = H.to_device(a).view(torch.int32) ^ 0x5A5A5A5A
    torch.cuda.synchronize()
    for _ in range(4):                                                      # work in front of the write, so that the call is enqueued behind it
        src = (src ^ 0x1111) ^ 0x1111
    tb.t.view(torch.int32).copy_(src ^ 0x5A5A5A5A)
    bufs = _call(gpu, tb, 9, True, 4)
    tb.a = a                                                                # (what the producer wrote)
    _verify(gpu, tb, 9, True, 4, bufs, "behind a producer")


def test_two_calls_back_to_back_on_one_scratch(gpu):
    import torch
    bm = gpu.topk_segments_limits("uint64", 0)[1]
    off1, n1 = S.residue_table([3, 700, bm + 9, 3 * bm + 1], 8)
    off2, n2 = S.residue_table([2 * bm + 3, 1, 513, bm + 1], 8)
    t1, t2 = Table(S.keys_for(n1, "uint64", 1), off1), Table(S.keys_for(n2, "uint64", 2), off2)
    k1, k2 = bm + 1, 40                                                     # (k1: the far class, whose part of the scratch lies behind the table)
    need = max(gpu.topk_segments_scratch_bytes(t1.n_seg, t1.longest, k1, "uint64"), gpu.topk_segments_scratch_bytes(t2.n_seg, t2.longest, k2, "uint64"))
    scratch = torch.full((need + 2 * SLACK,), POISON, dtype=torch.uint8, device="cuda")
    b1 = _call(gpu, t1, k1, False, None, scratch)
    b2 = _call(gpu, t2, k2, True, None, scratch)
    b3 = _call(gpu, t1, k2, True, None, scratch)
    _verify(gpu, t1, k1, False, None, b1, "first of three")
    _verify(gpu, t2, k2, True, None, b2, "second of three")
    _verify(gpu, t1, k2, True, None, b3, "third of three")
